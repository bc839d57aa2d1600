// The pixel rules of a uint16 depth frame (the Kinect's own millimetres, sample_pipeline.py:21) in
// MonkeyDetector.calculateCoM and getCrop, stated once for the host crop (mp_crop.hip) and the
// device kernels (k_detect.hip, k_frame.hip).  numpy 1.x promotes a uint16 array with a Python float
// scalar to float64, so both rules compare in double; the value a rule stores goes back into the
// uint16 array.  Plain C++: a host program (the CPU test) includes the same text.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MP_U16_HD __host__ __device__
#else
#define MP_U16_HD
#endif

#include <cstdint>

namespace mpu16 {

// calculateCoM's `dc[dc < self.minDepth] = 0; dc[dc > self.maxDepth] = 0` (monkeydetector.py:74-75):
// whether pixel v is zeroed
MP_U16_HD inline bool com_out(uint16_t v, double min_depth, double max_depth) {
  return (double)v < min_depth || (double)v > max_depth;
}

// The same threshold as integer bounds, computed once per launch: !com_out(v) <=> lo <= v <= hi.
// For an integer v, (double)v < a <=> v < ceil(a) and (double)v > b <=> v > floor(b); a bound the
// pixel range [0, 65535] cannot reach is clamped just outside it, and a NaN bound (every comparison
// with it is false) zeroes nothing.  min > max leaves lo > hi: every pixel is zeroed.
struct ComBounds {
  int32_t lo, hi;
};
MP_U16_HD inline ComBounds com_bounds(double min_depth, double max_depth) {
  ComBounds b;
  if (!(min_depth > 0.0))
    b.lo = 0;                                   // also NaN
  else if (min_depth > 65535.0)
    b.lo = 65536;
  else {
    b.lo = (int32_t)min_depth;                  // truncation = floor here
    if ((double)b.lo < min_depth) ++b.lo;       // ceil
  }
  if (!(max_depth < 65535.0))
    b.hi = 65535;                               // also NaN
  else if (max_depth < 0.0)
    b.hi = -1;
  else
    b.hi = (int32_t)max_depth;                  // floor
  return b;
}
MP_U16_HD inline bool com_out(uint16_t v, ComBounds b) { return (int32_t)v < b.lo || (int32_t)v > b.hi; }

// getCrop's thresholding (monkeydetector.py:208-212) of one frame pixel: `cropped[msk1] = zstart`
// stores zstart truncated into the uint16 array (zstart within int64 range), `cropped[msk2] = 0.`
MP_U16_HD inline uint16_t crop_px(uint16_t v, double zstart, double zend) {
  if ((double)v < zstart && v != 0) return (uint16_t)(int64_t)zstart;
  if ((double)v > zend && v != 0) return 0;
  return v;
}

}  // namespace mpu16
