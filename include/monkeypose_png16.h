/* monkeypose_png16.h -- PNG files from 16-bit depth frames, on the device and on the host
 * (libmonkeypose.so).
 *
 * The other direction of monkeypose_pngdec.h: uint16 frames go in, n finished 16-bit grayscale PNG
 * files come out -- the format of the importer's depth_*.png, which mp_png_decode_* reads back -- and
 * only their compressed bytes need to cross to the host.  The conventions of monkeypose.h hold (status
 * codes, mp_last_error, "asynchronous on `stream`" means ordered).
 *
 * The format is fixed to the byte by csrc/png16_rule.hpp, which the host encoder and the kernels both
 * read; mp_png16_encode_host is the reference of mp_png16_encode_dev, byte for byte.  In short:
 *   - signature, IHDR (bit depth 16, colour type 0, not interlaced), one IDAT per band, one 4-byte IDAT
 *     with the Adler-32, IEND.  Band 0's IDAT starts with the zlib header 78 01.
 *   - a row is a filter byte and 2 w big-endian bytes.  The filter is chosen per row among None, Sub,
 *     Up, Average and Paeth (bpp 2): the smallest sum of |residual byte as int8|, ties to the smallest
 *     filter number; the row above row 0 is zeros, and a band's first row is filtered against the
 *     frame's row above it.
 *   - the filtered stream is cut into bands of max(1, 8192 / (1 + 2 w)) whole rows; a band is
 *     compressed from that band alone.
 *   - tokens: greedy, left to right; at each position the longest match (3..258 bytes, inside the
 *     band) among the distances 1, 2, 4, 2 w - 1, 2 w + 1 and 2 w + 3 (a run, the two pixels before, the
 *     pixel above and its neighbours), ties to the smallest distance; else a literal.
 *   - a band is one stored, one fixed-Huffman or one dynamic-Huffman block, whichever is shortest
 *     (ties: fixed, then stored), followed by an empty stored block that ends on a byte boundary;
 *     the last one carries BFINAL.  The dynamic code's lengths come from the band's token counts by
 *     the one construction png16_rule.hpp states (15 bits at most; 7 for the code-length code).
 *
 * frames [n][h][w] uint16 in native byte order (2-byte aligned)
 * out    [n][out_stride] uint8 at any byte address, out_stride >= mp_png16_bound(h, w); frame i's file
 *        is out[i][0 .. sizes[i]); no other byte of out is written
 * sizes  [n] int64 (8-byte aligned)
 * work   mp_png16_work_bytes(n, h, w) bytes of device scratch, 16-byte aligned
 * stats  [n][mp_png16_band_count(h, w)][MP_PNG16_STAT_INTS] int32 (4-byte aligned), per band:
 *        [0] the form chosen (0 stored, 1 fixed, 2 dynamic), [1..5] the rows that took filter 0..4,
 *        [6] the matches, [7] the distinct distance symbols, [8] the depth of the deeper of the
 *        literal/length and distance Huffman trees before the 15-bit limit
 * Limits: 1 <= n <= 65535 and 1 <= h, w <= 4096.  MP_ERR_SHAPE: n, h, w or out_stride out of range;
 * MP_ERR_ARG: a null or misaligned pointer.  Both before any launch, out and sizes untouched.
 * mp_png16_bound, mp_png16_work_bytes, mp_png16_band_rows and mp_png16_band_count return 0 for a
 * shape out of range.
 *
 * mp_png16_encode_dev takes device pointers, allocates nothing, waits for nothing and is ordered on
 * `stream`.  mp_png16_encode_host and mp_png16_band_stats_host take host pointers and run the same
 * rule on the calling thread.
 */
#ifndef MONKEYPOSE_PNG16_H
#define MONKEYPOSE_PNG16_H

#include "monkeypose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MP_PNG16_STAT_INTS 9

/* bytes of one frame's worst-case file (every band stored); sizes[i] <= mp_png16_bound(h, w) */
size_t mp_png16_bound(int64_t h, int64_t w);
/* device scratch of mp_png16_encode_dev */
size_t mp_png16_work_bytes(int64_t n, int64_t h, int64_t w);
/* rows of each band, and the number of bands of an h x w frame (the plan the bytes follow) */
int mp_png16_band_rows(int64_t w);
int mp_png16_band_count(int64_t h, int64_t w);

int mp_png16_encode_host(const uint16_t* frames, int64_t n, int64_t h, int64_t w, uint8_t* out,
                         int64_t out_stride, int64_t* sizes);
int mp_png16_encode_dev(const uint16_t* frames, int64_t n, int64_t h, int64_t w, uint8_t* out,
                        int64_t out_stride, int64_t* sizes, void* work, void* stream);
int mp_png16_band_stats_host(const uint16_t* frames, int64_t n, int64_t h, int64_t w, int32_t* stats);

#ifdef __cplusplus
}
#endif

#endif /* MONKEYPOSE_PNG16_H */
