/* monkeypose_png.h -- PNG files from RGB pictures, on the device and on the host (libmonkeypose.so).
 *
 * The last step of the picture path: mp_overlay_dev's out[n][h][w][3] goes in, n finished PNG files
 * come out, and only their compressed bytes need to cross to the host.  The conventions of
 * monkeypose.h hold (status codes, mp_last_error, "asynchronous on `stream`" means ordered).
 *
 * The format is fixed to the byte by csrc/png_rule.hpp, which the host encoder and the kernels both
 * read; mp_png_encode_host is the reference of mp_png_encode_dev, byte for byte.  In short:
 *   - signature, IHDR (8-bit RGB, not interlaced), one IDAT per band, one 4-byte IDAT with the
 *     Adler-32, IEND.  Band 0's IDAT starts with the zlib header 78 01.
 *   - rows carry filter byte 0.  The raw stream is cut into bands of max(1, 8192 / (1 + 3 w)) whole
 *     rows; a band is compressed from that band alone.
 *   - a band is one fixed-Huffman block or one stored block, whichever is shorter (ties: fixed),
 *     followed by an empty stored block that ends on a byte boundary; the last one carries BFINAL.
 *   - tokens: greedy, left to right; at each position the longest match (3..258 bytes, inside the
 *     band) among the distances 1, 3, 6, 3 w - 2, 3 w + 1 and 3 w + 4 (a run, the two pixels before, the
 *     pixel above and its neighbours), ties to the smallest distance; else a literal.
 *
 * rgb   [n][h][w][3] uint8 at any byte address
 * out   [n][out_stride] uint8 at any byte address, out_stride >= mp_png_bound(h, w); image i's file is
 *       out[i][0 .. sizes[i]); no other byte of out is written
 * sizes [n] int64 (8-byte aligned)
 * work  mp_png_work_bytes(n, h, w) bytes of device scratch, 16-byte aligned
 * Limits: 1 <= n <= 65535 and 1 <= h, w <= 4096.  MP_ERR_SHAPE: n, h, w or out_stride out of range;
 * MP_ERR_ARG: a null or misaligned pointer.  Both before any launch, out and sizes untouched.
 * mp_png_bound and mp_png_work_bytes return 0 for a shape out of range.
 *
 * mp_png_encode_dev takes device pointers, allocates nothing, waits for nothing and is ordered on
 * `stream`.  mp_png_encode_host takes host pointers and runs the same rule on the calling thread.
 */
#ifndef MONKEYPOSE_PNG_H
#define MONKEYPOSE_PNG_H

#include "monkeypose.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of one image's worst-case file (every band stored); sizes[i] <= mp_png_bound(h, w) */
size_t mp_png_bound(int64_t h, int64_t w);
/* device scratch of mp_png_encode_dev */
size_t mp_png_work_bytes(int64_t n, int64_t h, int64_t w);
/* raw rows of each band, and the number of bands of an h x w image (the plan the bytes follow) */
int mp_png_band_rows(int64_t w);
int mp_png_band_count(int64_t h, int64_t w);

int mp_png_encode_host(const uint8_t* rgb, int64_t n, int64_t h, int64_t w, uint8_t* out, int64_t out_stride,
                       int64_t* sizes);
int mp_png_encode_dev(const uint8_t* rgb, int64_t n, int64_t h, int64_t w, uint8_t* out, int64_t out_stride,
                      int64_t* sizes, void* work, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MONKEYPOSE_PNG_H */
