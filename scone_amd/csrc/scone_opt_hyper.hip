// The optimizer's hyper-parameter block on the device (include/scone_hip.h, "optimizer hyper-parameters on the device"):
// scone_opt_hyper_init writes the 104 bytes, scone_opt_hyper_advance counts an applied step and derives the fp32 scalars the step
// kernels read (k_opt_step / k_opt_lean instantiated with opt_s_device, scone_opt_rows.h), and scone_opt_hyper_scalars_of is the
// host copy of that derivation.
//
// One definition, two compilers.  hyper_scalars is __host__ __device__: the host copy and the device kernel are the same source,
// every operation one IEEE double rounding -- built with -ffp-contract=off, sqrt and / correctly rounded on both sides (the
// device's as k_grad_ctl_set relies on), no libm call.  Adam's powers are the integer power the header states, not pow(): a
// pure function of (beta, t) on every machine.
//
// Both kernels are one thread; all stores are plain stores of that thread.
#include "scone_common.h"
#include "scone_opt_rows.h"  // opt_cfg_check

#include <cmath>
#include <cstddef>

static_assert(sizeof(scone_opt_hyper) == 104 && offsetof(scone_opt_hyper, seed) == 48 && offsetof(scone_opt_hyper, step) == 56 &&
                  offsetof(scone_opt_hyper, sc) == 64 && offsetof(scone_opt_hyper, applied) == 96 && offsetof(scone_opt_hyper, bad) == 100,
              "scone_opt_hyper is 104 bytes with the offsets of include/scone_hip.h");

namespace {

// the header's ipow: every product one IEEE double
__host__ __device__ inline double hyper_ipow(double b, unsigned long long t) {
  double r = 1.0;
  while (t) {
    if (t & 1ull) r = r * b;
    t >>= 1;
    if (t) b = b * b;
  }
  return r;
}

__host__ __device__ inline scone_opt_scalars hyper_scalars(int kind, double lr, double beta1, double beta2, double eps, double weight_decay,
                                                           double grad_scale, long long step) {
  double alpha = lr;
  if (kind == SCONE_OPT_ADAM) {
    const unsigned long long t = (unsigned long long)step;
    const double p2 = hyper_ipow(beta2, t), p1 = hyper_ipow(beta1, t);
    const double num = lr * sqrt(1.0 - p2);
    alpha = num / (1.0 - p1);
  }
  scone_opt_scalars out;
  out.alpha = (float)alpha;
  out.b1 = (float)beta1;
  out.b2 = (float)beta2;
  out.c1 = (float)(1.0 - beta1);
  out.c2 = (float)(1.0 - beta2);
  out.eps = (float)eps;
  out.decay = (float)(lr * weight_decay);
  out.gscale = (float)grad_scale;
  return out;
}

__device__ __forceinline__ bool hyper_finite(double x) {
  return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

__global__ void k_opt_hyper_init(scone_opt_hyper *__restrict__ hy, double lr, double beta1, double beta2, double eps, double weight_decay,
                                 double grad_scale, unsigned long long seed, long long step) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  hy->lr = lr, hy->beta1 = beta1, hy->beta2 = beta2, hy->eps = eps, hy->weight_decay = weight_decay, hy->grad_scale = grad_scale;
  hy->seed = seed;
  hy->step = step;
  hy->sc = scone_opt_scalars{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  hy->applied = 0u;
  hy->bad = 0u;
}

__global__ void k_opt_hyper_advance(scone_opt_hyper *__restrict__ hy, int kind, const scone_grad_ctl *__restrict__ ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (ctl && ctl->skip != 0u) {  // the step is skipped: it is not counted
    hy->applied = 0u;
    return;
  }
  const double lr = hy->lr, beta1 = hy->beta1, beta2 = hy->beta2, eps = hy->eps, wd = hy->weight_decay, gs = hy->grad_scale;
  const long long step = hy->step;
  if (!hyper_finite(lr) || !hyper_finite(beta1) || !hyper_finite(beta2) || !hyper_finite(eps) || !hyper_finite(wd) || !hyper_finite(gs) ||
      step == 0x7FFFFFFFFFFFFFFFll) {
    hy->applied = 0u;
    hy->bad = 1u;
    return;
  }
  hy->step = step + 1;
  hy->sc = hyper_scalars(kind, lr, beta1, beta2, eps, wd, gs, step + 1);
  hy->applied = 1u;
  hy->bad = 0u;
}

bool hyper_kind_ok(int32_t kind) { return kind == SCONE_OPT_SGD || kind == SCONE_OPT_ADAGRAD || kind == SCONE_OPT_ADAM; }

}  // namespace

extern "C" int scone_opt_hyper_scalars_of(const scone_opt_cfg *cfg, scone_opt_scalars *out) {
  if (!out || opt_cfg_check(cfg)) return SCONE_EINVAL;
  *out = hyper_scalars(cfg->kind, cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->weight_decay, cfg->grad_scale, cfg->step);
  return SCONE_OK;
}

extern "C" int scone_opt_hyper_init(scone_handle *h, const scone_opt_cfg *cfg, uint64_t seed, scone_opt_hyper *d_hyper, void *stream) {
  const char *who = "scone_opt_hyper_init";
  if (!h) return SCONE_EINVAL;
  if (const char *bad = opt_cfg_check(cfg, false)) return scone_refuse(h, SCONE_EINVAL, who, bad);
  if (cfg->step < 0) return scone_refuse(h, SCONE_EINVAL, who, "step is the number of steps already applied: it must be >= 0");
  if (!d_hyper) return scone_refuse(h, SCONE_EINVAL, who, "null d_hyper");
  SCONE_ON_DEVICE(h);
  hipLaunchKernelGGL(k_opt_hyper_init, dim3(1), dim3(1), 0, (hipStream_t)stream, d_hyper, cfg->lr, cfg->beta1, cfg->beta2, cfg->eps,
                     cfg->weight_decay, cfg->grad_scale, (unsigned long long)seed, (long long)cfg->step);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}

extern "C" int scone_opt_hyper_advance(scone_handle *h, int32_t kind, scone_opt_hyper *d_hyper, const scone_grad_ctl *d_ctl, void *stream) {
  const char *who = "scone_opt_hyper_advance";
  if (!h) return SCONE_EINVAL;
  if (!hyper_kind_ok(kind)) return scone_refuse(h, SCONE_EINVAL, who, "bad kind");
  if (!d_hyper) return scone_refuse(h, SCONE_EINVAL, who, "null d_hyper");
  SCONE_ON_DEVICE(h);
  hipLaunchKernelGGL(k_opt_hyper_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, d_hyper, (int)kind, d_ctl);
  SCONE_HIP(h, hipGetLastError());
  return SCONE_OK;
}
