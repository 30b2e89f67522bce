// The reference driver's other two optimizers (train.py:286-290) on the flat fp32 buffers of optimizer.hip, fused with the
// gradient clip exactly as adam_kernel is: the gradient is scaled by norm_and_coef[1] (vqa_grad_norm_clip_coef) as it is read.
//
//   SGD, momentum mu (torch.optim.SGD, dampening 0, no Nesterov, no weight decay):
//       buf = mu * buf + g ; p -= lr * buf
//     torch seeds buf with a copy of g at the first step; a zero-initialised buf gives exactly that (mu * 0 + g), so there is
//     no step branch and no step count.
//   RMSprop (torch.optim.RMSprop defaults: momentum 0, not centered):
//       sq = alpha * sq + (1 - alpha) * g^2 ; p -= lr * g / (sqrt(sq) + eps)
//
// One pass that reads p, g and the one state buffer and writes p and the state: 20 B per parameter against Adam's 28.
// adam_kernel's launch geometry: 256 threads, one float4 per thread, the scalar tail on the thread that meets the end.
// `dyn` (optional, device): {lr} -- word 0 of the trainer's per-step block, so a captured hipGraph of the step can be replayed
// while the learning rate moves on.
#include "common.hpp"

namespace vqa {

enum { kSgd = 0, kRms = 1 };

// h = mu (SGD) or alpha (RMSprop); omh = 1 - alpha and eps are read by RMSprop only.  1 - alpha is rounded from the double
// on the host, as torch rounds the two scalars of mul_(alpha).addcmul_(g, g, value=1 - alpha) separately: 1.f - 0.99f is
// 1e-6 away from 0.01f, and that error would sit in every square average.
template <int KIND>
__device__ __forceinline__ void state_step(float& p, float& s, float g, float lr, float h, float omh, float eps) {
  if (KIND == kSgd) {
    s = h * s + g;
    p -= lr * s;
  } else {
    s = h * s + omh * g * g;
    p -= lr * g / (sqrtf(s) + eps);
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void state_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ st,
                                                         size_t n, const float* __restrict__ coef_ptr,
                                                         const float* __restrict__ dyn, float lr, float h, float omh, float eps) {
  const float coef = coef_ptr != nullptr ? coef_ptr[1] : 1.f;
  if (dyn != nullptr) lr = dyn[0];
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) {
    const float4 gg = ld4(g + i);
    float4 pp = ld4(p + i), ss = ld4(st + i);
    state_step<KIND>(pp.x, ss.x, gg.x * coef, lr, h, omh, eps);
    state_step<KIND>(pp.y, ss.y, gg.y * coef, lr, h, omh, eps);
    state_step<KIND>(pp.z, ss.z, gg.z * coef, lr, h, omh, eps);
    state_step<KIND>(pp.w, ss.w, gg.w * coef, lr, h, omh, eps);
    st4(p + i, pp);
    st4(st + i, ss);
  } else {
    for (size_t j = i; j < n; ++j) {
      float pj = p[j], sj = st[j];
      state_step<KIND>(pj, sj, g[j] * coef, lr, h, omh, eps);
      p[j] = pj;
      st[j] = sj;
    }
  }
}

template <int KIND>
static int launch_step(const char* what, float* p, const float* g, float* st, size_t n, const float* norm_and_coef,
                       const float* step_scalars, bool dyn, float lr, float h, float omh, float eps, vqa_stream_t stream) {
  VQA_REQUIRE(p && g && st && (step_scalars || !dyn) && n > 0, VQA_E_BADARG, "%s: null pointer or n == 0", what);
  VQA_REQUIRE(aligned(p, 16) && aligned(g, 16) && aligned(st, 16), VQA_E_UNSUPPORTED, "%s: buffers must be 16-byte aligned", what);
  const size_t blocks = (n / 4 + 256) / 256;
  VQA_REQUIRE(blocks <= 0x7fffffffu, VQA_E_UNSUPPORTED, "%s: n=%zu exceeds the launch grid", what, n);
  VQA_LAUNCH(state_step_kernel<KIND>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, st, n,
             norm_and_coef, step_scalars, lr, h, omh, eps);
  return check_launch(what);
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_sgd_step(float* p, const float* g, float* buf, size_t n, const float* norm_and_coef, float lr, float momentum,
                            vqa_stream_t stream) {
  return launch_step<kSgd>("sgd_step", p, g, buf, n, norm_and_coef, nullptr, false, lr, momentum, 0.f, 0.f, stream);
}

extern "C" int vqa_sgd_step_dyn(float* p, const float* g, float* buf, size_t n, const float* norm_and_coef,
                                const float* step_scalars, float momentum, vqa_stream_t stream) {
  return launch_step<kSgd>("sgd_step_dyn", p, g, buf, n, norm_and_coef, step_scalars, true, 0.f, momentum, 0.f, 0.f, stream);
}

extern "C" int vqa_rmsprop_step(float* p, const float* g, float* sq, size_t n, const float* norm_and_coef, float lr, double alpha,
                                float eps, vqa_stream_t stream) {
  return launch_step<kRms>("rmsprop_step", p, g, sq, n, norm_and_coef, nullptr, false, lr, (float)alpha, (float)(1.0 - alpha), eps, stream);
}

extern "C" int vqa_rmsprop_step_dyn(float* p, const float* g, float* sq, size_t n, const float* norm_and_coef,
                                    const float* step_scalars, double alpha, float eps, vqa_stream_t stream) {
  return launch_step<kRms>("rmsprop_step_dyn", p, g, sq, n, norm_and_coef, step_scalars, true, 0.f, (float)alpha, (float)(1.0 - alpha), eps, stream);
}
