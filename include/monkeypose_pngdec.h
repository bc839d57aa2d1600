/* monkeypose_pngdec.h -- PNG files to pixels, on the device and on the host (libmonkeypose.so).
 *
 * The first step of the frame path: n PNG files of one shape go in (the reference's depth_*.png are
 * 16-bit grayscale), their pixels come out, and only the compressed bytes need to cross to the
 * device.  The conventions of monkeypose.h hold (status codes, mp_last_error, "asynchronous on
 * `stream`" means ordered).
 *
 * The rule is csrc/pngdec_rule.hpp, which the host decoder and the kernels both read; there is no zlib
 * in the library.  mp_png_decode_host is the reference of mp_png_decode_dev, bit for bit, in the
 * pixels and in the statuses.  In short:
 *   - container: the signature; chunks of length, type, data, CRC-32, every CRC checked; IHDR first,
 *     IEND last and empty, at least one IDAT and the IDATs consecutive (a zero-length one is legal);
 *     PLTE accepted before them and ignored; ancillary chunks skipped; any other critical chunk
 *     refused.
 *   - formats: MP_PNG_GRAY16 (colour type 0, depth 16) -> uint16 [n][h][w] in host byte order,
 *     MP_PNG_GRAY8 (0, 8) -> uint8 [n][h][w], MP_PNG_RGB8 (2, 8) -> uint8 [n][h][w][3] (what
 *     mp_png_encode_* writes).  Interlace, palette, alpha, depths below 8, 16-bit RGB and a
 *     compression or filter method other than 0 are "unsupported".
 *   - zlib / deflate (RFC 1950 / 1951) in full: stored, fixed and dynamic blocks in any mix, code
 *     sets by zlib's own verdicts, the Adler-32 checked, exactly h (1 + row bytes) bytes of output.
 *   - filter types 0..4 per row.
 *
 * status[i] (int32) is 0 for a decoded file, else the first failure in this order:
 *   1 container   2 CRC   3 unsupported   4 the file's h, w or format is not the call's
 *   5 deflate / zlib stream   6 Adler-32   7 filter byte
 * A failed file's image is all zeros, and it never disturbs its neighbours in the batch.  No byte
 * sequence makes the decoder read or write outside what the call was given, or loop without end.
 *
 * files  [n][file_stride] uint8 at any byte address; file i is files[i][0 .. sizes[i])
 * sizes  [n] int64 (8-byte aligned), 0 <= sizes[i] <= file_stride (a size outside that range: the
 *        file's status is 1)
 * out    the images, aligned to their element (2 bytes for MP_PNG_GRAY16)
 * status [n] int32 (4-byte aligned)
 * work   mp_png_decode_work_bytes(n, h, w, format, file_stride) bytes of device scratch, 16-byte aligned
 * Limits: 1 <= n <= 65535, 1 <= h, w <= 4096, 1 <= file_stride <= 2^30.  MP_ERR_SHAPE: n, h, w, format
 * or file_stride out of range; MP_ERR_ARG: a null or misaligned pointer.  Both before any launch, out
 * and status untouched.  mp_png_decode_work_bytes returns 0 for a shape out of range.  Both decode
 * calls return MP_OK when the call ran, whatever the files' statuses.
 *
 * mp_png_decode_dev takes device pointers, allocates nothing, waits for nothing and is ordered on
 * `stream`; nothing outside out, status and work is written.  mp_png_decode_host takes host pointers
 * and runs the same rule on the calling thread.
 */
#ifndef MONKEYPOSE_PNGDEC_H
#define MONKEYPOSE_PNGDEC_H

#include "monkeypose.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MP_PNG_GRAY16 = 0, MP_PNG_GRAY8 = 1, MP_PNG_RGB8 = 2 };

/* device scratch of mp_png_decode_dev */
size_t mp_png_decode_work_bytes(int64_t n, int64_t h, int64_t w, int format, int64_t file_stride);

int mp_png_decode_host(const uint8_t* files, int64_t file_stride, const int64_t* sizes, int64_t n, int64_t h, int64_t w,
                       int format, void* out, int32_t* status);
int mp_png_decode_dev(const uint8_t* files, int64_t file_stride, const int64_t* sizes, int64_t n, int64_t h, int64_t w,
                      int format, void* out, int32_t* status, void* work, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MONKEYPOSE_PNGDEC_H */
