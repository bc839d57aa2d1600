// C ABI of the validation pass on the device (k_eval.hip): argument checks on the host, then
// asynchronous launches on the caller's stream.  Nothing is allocated and nothing synchronises.
#include "eval_plan.hpp"
#include "mp_kernels.hpp"
#include "mp_runtime.hpp"

namespace {

void check_cam(const mp_camera* cam) {
  if (!cam) fail(MP_ERR_ARG, "camera is NULL");
  if (!(cam->fx > 0) || !(cam->fy > 0) || !(cam->cube[0] > 0) || !(cam->cube[1] > 0) || !(cam->cube[2] > 0))
    fail(MP_ERR_ARG, "camera focal lengths and cube must be positive");
}

bool shape_ok(int64_t n, int64_t joints) {
  return n > 0 && n <= 65535 && joints > 0 && joints <= evalplan::MAX_JOINTS;
}

bool state_shape_ok(int64_t joints, int64_t T) {
  return joints > 0 && joints <= evalplan::MAX_JOINTS && T >= 0 && T <= evalplan::MAX_THRESHOLDS;
}

void check_state(const char* who, const void* state, int64_t joints, int64_t T) {
  if (!state) fail(MP_ERR_ARG, std::string(who) + ": null pointer");
  if (!state_shape_ok(joints, T))
    fail(MP_ERR_SHAPE, std::string(who) + ": joints must be 1..128 and T 0..1024");
  if (reinterpret_cast<uintptr_t>(state) & 7) fail(MP_ERR_ARG, std::string(who) + ": state must be 8-byte aligned");
}

}  // namespace

extern "C" {

int mp_rel_labels_dev(const mp_camera* cam, const float* labels, int64_t n, int64_t joints, const double* coms,
                      float* rel, void* stream) {
  return guard([&] {
    check_cam(cam);
    if (!labels || !coms || !rel) fail(MP_ERR_ARG, "mp_rel_labels_dev: null pointer");
    if (!shape_ok(n, joints)) fail(MP_ERR_SHAPE, "mp_rel_labels_dev: bad shape (n <= 65535, joints <= 128)");
    hip_check(mp::launch_rel_labels(*cam, labels, n, (int)joints, coms, rel, static_cast<hipStream_t>(stream)),
              "rel_labels");
  });
}

int mp_com_from_joints_dev(const mp_camera* cam, const float* labels, int64_t n, int64_t joints, double scale_u,
                           double scale_v, double scale_d, float* com, void* stream) {
  return guard([&] {
    check_cam(cam);
    if (!labels || !com) fail(MP_ERR_ARG, "mp_com_from_joints_dev: null pointer");
    if (!shape_ok(n, joints)) fail(MP_ERR_SHAPE, "mp_com_from_joints_dev: bad shape (n <= 65535, joints <= 128)");
    hip_check(mp::launch_com_from_joints(*cam, labels, n, (int)joints, (float)scale_u, (float)scale_v, (float)scale_d,
                                         com, static_cast<hipStream_t>(stream)),
              "com_from_joints");
  });
}

size_t mp_eval_state_bytes(int64_t joints, int64_t T) {
  return state_shape_ok(joints, T) ? mp::eval_state_bytes((int)joints, (int)T) : 0;
}

size_t mp_eval_work_bytes(int64_t n, int64_t joints) {
  return shape_ok(n, joints) ? mp::eval_work_bytes(n, (int)joints) : 0;
}

int64_t mp_eval_summary_len(int64_t joints, int64_t T) { return state_shape_ok(joints, T) ? 4 + joints + 2 * T : 0; }

int mp_eval_reset_dev(void* state, int64_t joints, int64_t T, const float* thresholds, void* stream) {
  return guard([&] {
    check_state("mp_eval_reset_dev", state, joints, T);
    if (T > 0 && !thresholds) fail(MP_ERR_ARG, "mp_eval_reset_dev: thresholds is NULL");
    hip_check(mp::launch_eval_reset(state, (int)joints, (int)T, thresholds, static_cast<hipStream_t>(stream)),
              "eval_reset");
  });
}

int mp_eval_accumulate_dev(void* state, const float* labels, const float* results, int64_t n, int64_t joints,
                           int64_t T, float scale, void* work, size_t work_bytes, float* dist, float* frame_mean,
                           float* frame_max, void* stream) {
  return guard([&] {
    check_state("mp_eval_accumulate_dev", state, joints, T);
    if (!labels || !results || !work) fail(MP_ERR_ARG, "mp_eval_accumulate_dev: null pointer");
    if (!shape_ok(n, joints)) fail(MP_ERR_SHAPE, "mp_eval_accumulate_dev: bad shape (n <= 65535, joints <= 128)");
    if (work_bytes < mp::eval_work_bytes(n, (int)joints))
      fail(MP_ERR_ARG, "mp_eval_accumulate_dev: work buffer smaller than mp_eval_work_bytes()");
    if (reinterpret_cast<uintptr_t>(work) & 7) fail(MP_ERR_ARG, "mp_eval_accumulate_dev: work must be 8-byte aligned");
    float* w = static_cast<float*>(work);
    float* d = dist ? dist : w;
    float* fm = frame_mean ? frame_mean : w + n * joints;
    float* fx = frame_max ? frame_max : w + n * joints + n;
    hip_check(mp::launch_eval_accumulate(state, labels, results, n, (int)joints, (int)T, scale, d, fm, fx,
                                         static_cast<hipStream_t>(stream)),
              "eval_accumulate");
  });
}

int mp_eval_summary_dev(const void* state, int64_t joints, int64_t T, double* out, void* stream) {
  return guard([&] {
    check_state("mp_eval_summary_dev", state, joints, T);
    if (!out) fail(MP_ERR_ARG, "mp_eval_summary_dev: null pointer");
    hip_check(mp::launch_eval_summary(state, (int)joints, (int)T, out, static_cast<hipStream_t>(stream)),
              "eval_summary");
  });
}

}  // extern "C"
