// The step epilogue: what follows the UNet in every denoising step, one launch per step for every sampler.  The shared body owns the read of the
// device step counter, the grid-stride loop, the CFG combine, the frozen-mask blend, the `latents` and history stores and the next UNet input
// (written twice, in the model dtype).  A sampler is an update policy: its coefficient row and the arithmetic between the combined model output and
// the new latents.  tg_step_epilogue (DDIM), tg_step_epilogue_sigma (Euler / Euler ancestral) and tg_step_epilogue_dpm (DPM-Solver++ multistep)
// are the three policies below; a further sampler is one more policy and one more entry point.  HBM-bound, about 4 us at the flagship shape.
#include "tg_common.h"

namespace {

// what every sampler's launch shares (host side: the entry points fill it, launch_step checks it)
struct StepCommon {
  const float* noise_pred;    // [2 * n_img * chw] (uncond half first) when has_cfg, else [n_img * chw]
  float* latents;             // [n_img * chw], updated in place
  int n_img, chw, hw;
  int has_cfg;
  float g;
  const float* coef;          // [n_steps][row of the policy]
  int* step_idx;
  const float* frozen;        // [n_steps + 1][n_img * chw] or null
  const float* frozen_mask;   // [n_img | 1][hw]
  int mask_per_img;
  int frozen_steps;
  float* history;             // [n_steps + 1][n_img * chw] or null
  void* model_in;             // [2][n_img * chw] in model_in_dtype, or null
  int model_in_dtype;
};

// An update policy supplies
//   Row row(coef, step)                      this step's coefficients, loaded once per thread before the loop
//   float next(row, x, m, step, total, i)    the new latent of element i from the old one `x` and the (CFG-combined) model output `m`; it may
//                                            read and write per-element state of its own at i (element i is visited by one thread only)
//   float input(row, nx)                     the next UNet input from the (blended) new latent
// and nothing else: no loop, no blend, no store into the shared buffers.

// DDIM (eta = 0): row = sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)
struct DdimUpdate {
  int pred_type;              // 0 = epsilon, 1 = v_prediction
  struct Row { float sa, sb, sap, sbp; };
  __device__ __forceinline__ Row row(const float* coef, int step) const {
    return Row{coef[step * 4], coef[step * 4 + 1], coef[step * 4 + 2], coef[step * 4 + 3]};
  }
  __device__ __forceinline__ float next(const Row& r, float x, float mo, int, long, long) const {
    float x0, eps;
    if (pred_type == 0) { x0 = (x - r.sb * mo) / r.sa; eps = mo; }
    else { x0 = r.sa * x - r.sb * mo; eps = r.sa * mo + r.sb * x; }
    return r.sap * x0 + r.sbp * eps;
  }
  // next UNet input = cat([latents] * 2) in the model dtype (models/pipelines.py:409-414)
  __device__ __forceinline__ float input(const Row&, float nx) const { return nx; }
};

__device__ __forceinline__ float load_any(const void* p, int dt, long i) {
  if (dt == TG_BF16) return (float)reinterpret_cast<const bf16_t*>(p)[i];
  if (dt == TG_F16) return (float)reinterpret_cast<const f16_t*>(p)[i];
  return reinterpret_cast<const float*>(p)[i];
}

// Euler / Euler ancestral: row = eps weight, sigma_up, scale of the next model input, sigma_i (informational)
struct SigmaUpdate {
  const void* noise;          // [n_steps][n_img * chw] in noise_dtype, or null (sigma_up ignored)
  int noise_dtype;
  struct Row { float ce, su, cnext; };
  __device__ __forceinline__ Row row(const float* coef, int step) const {
    return Row{coef[step * 4], coef[step * 4 + 1], coef[step * 4 + 2]};
  }
  __device__ __forceinline__ float next(const Row& r, float x, float eps, int step, long total, long i) const {
    float nx = x + eps * r.ce;
    if (noise) nx += r.su * load_any(noise, noise_dtype, (long)step * total + i);
    return nx;
  }
  // next UNet input = scale_model_input(cat([latents] * 2), t_next) = x / sqrt(sigma_next^2 + 1), in the model dtype; PyTorch divides a
  // tensor by a scalar as a multiply by the fp32 reciprocal, which the table holds
  __device__ __forceinline__ float input(const Row& r, float nx) const { return nx * r.cnext; }
};

// DPM-Solver++ multistep (data prediction, midpoint 2M): x0 = cx x + ce m, x' = A x + B x0 + C x0_prev with the row (cx, ce, A, B, C, 0, 0, 0) of
// this step.  C == 0 marks a first-order row: the state is then NOT read (0 * NaN of a never-written buffer would be NaN); the row is
// the same for every thread, so the branch is wave-uniform.  Each element of x0_prev is read and rewritten by one thread only.
struct DpmUpdate {
  float* x0_prev;             // [n_img * chw] fp32: the previous step's data prediction, replaced by this step's
  struct Row { float cx, ce, ca, cb, cc; bool second; };
  __device__ __forceinline__ Row row(const float* coef, int step) const {
    const float* r = coef + (long)step * 8;
    return Row{r[0], r[1], r[2], r[3], r[4], r[4] != 0.f};
  }
  __device__ __forceinline__ float next(const Row& r, float x, float m, int, long, long i) const {
    const float x0 = r.cx * x + r.ce * m;
    float nx = r.ca * x + r.cb * x0;
    if (r.second) nx += r.cc * x0_prev[i];
    x0_prev[i] = x0;                       // the model's prediction, not the blended latents (host loop: scheduler.step, then the blend)
    return nx;
  }
  // next UNet input = cat([latents] * 2) in the model dtype (scale_model_input is the identity: init_noise_sigma = 1)
  __device__ __forceinline__ float input(const Row&, float nx) const { return nx; }
};

// The kernel's argument: StepCommon's fields with the policy's own between `step_idx` and `frozen`.  That is the field order of the three kernels this
// body replaced, and it is kept on purpose: the compiler orders the scalar loads of the arguments ahead of the loop after the layout, and with the
// policy passed as a second argument the Euler-ancestral launch measured 1.1 % slower than its predecessor (and the DDIM launch 1.5 % faster) with an
// identical loop.  With this layout the argument loads and the launch times are the predecessors' (profiles/step_epilogue_unify_findings.md).
template <class Update>
struct StepArgs {
  const float* noise_pred;
  float* latents;
  int n_img, chw, hw;
  int has_cfg;
  float g;
  const float* coef;
  int* step_idx;
  Update up;
  const float* frozen;
  const float* frozen_mask;
  int mask_per_img;
  int frozen_steps;
  float* history;
  void* model_in;
  int model_in_dtype;
};

template <class Update>
__global__ __launch_bounds__(256) void step_epilogue_kernel(StepArgs<Update> p) {
  const int step = *p.step_idx;
  const typename Update::Row row = p.up.row(p.coef, step);
  const long total = (long)p.n_img * p.chw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const float u = p.noise_pred[i];
    float m = u;
    if (p.has_cfg) { const float c = p.noise_pred[total + i]; m = u + p.g * (c - u); }
    float nx = p.up.next(row, p.latents[i], m, step, total, i);
    if (p.frozen && step < p.frozen_steps) {
      const long img = i / p.chw;
      const long pix = (i - img * p.chw) % p.hw;
      const float mk = p.frozen_mask[(p.mask_per_img ? img * p.hw : 0) + pix];
      const float f = p.frozen[(long)(step + 1) * total + i];
      nx = f * mk + nx * (1.f - mk);
    }
    p.latents[i] = nx;
    if (p.history) p.history[(long)(step + 1) * total + i] = nx;
    if (p.model_in) {
      const float s = p.up.input(row, nx);
      if (p.model_in_dtype == TG_BF16) {
        reinterpret_cast<bf16_t*>(p.model_in)[i] = (bf16_t)s;
        reinterpret_cast<bf16_t*>(p.model_in)[total + i] = (bf16_t)s;
      } else if (p.model_in_dtype == TG_F16) {
        reinterpret_cast<f16_t*>(p.model_in)[i] = (f16_t)s;
        reinterpret_cast<f16_t*>(p.model_in)[total + i] = (f16_t)s;
      } else {
        reinterpret_cast<float*>(p.model_in)[i] = s;
        reinterpret_cast<float*>(p.model_in)[total + i] = s;
      }
    }
  }
}

__global__ void step_advance_kernel(int* step_idx) { *step_idx += 1; }

inline bool src_dtype_ok(int dt) { return dt == TG_BF16 || dt == TG_F16 || dt == 2; }

// the checks every entry point shares (`name` = the entry point, for the error text), the epilogue launch and the counter launch
template <class Update>
int launch_step(const char* name, const StepCommon& p, const Update& up, int advance, void* stream) {
  TG_CHECK(p.noise_pred && p.latents && p.coef && p.step_idx && p.n_img > 0 && p.chw > 0 && p.hw > 0 && p.chw % p.hw == 0, TG_ERR_ARG,
           "%s: bad args", name);
  TG_CHECK(!p.frozen || p.frozen_mask, TG_ERR_ARG, "%s: frozen latents need a mask", name);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(step_epilogue_kernel<Update>, dim3(tg_blocks_1d((long)p.n_img * p.chw)), dim3(256), 0, st,
                     StepArgs<Update>{p.noise_pred, p.latents, p.n_img, p.chw, p.hw, p.has_cfg, p.g, p.coef, p.step_idx, up, p.frozen, p.frozen_mask,
                                      p.mask_per_img, p.frozen_steps, p.history, p.model_in, p.model_in_dtype});
  TG_LAUNCH_CHECK();
  if (advance) {
    // a launch of its own, ordered after the epilogue on the stream: no thread of the epilogue can read a moved counter
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, st, p.step_idx);
    TG_LAUNCH_CHECK();
  }
  return TG_OK;
}

}  // namespace

extern "C" int tg_step_epilogue(const float* noise_pred, float* latents, int32_t n_img, int32_t chw, int32_t hw,
                                int32_t has_cfg, float guidance_scale, const float* coef, int32_t* step_idx, int32_t advance,
                                int32_t prediction_type, const float* frozen, const float* frozen_mask,
                                int32_t mask_per_img, int32_t frozen_steps, float* history, void* model_in,
                                int32_t model_in_dtype, void* stream) {
  TG_CHECK(prediction_type == 0 || prediction_type == 1, TG_ERR_ARG, "tg_step_epilogue: bad prediction type");
  // model_in_dtype is not checked here (it never was): any value other than TG_BF16 / TG_F16 stores fp32
  const StepCommon p{noise_pred, latents, n_img, chw, hw, has_cfg, guidance_scale, coef, step_idx, frozen,
                     frozen_mask, mask_per_img, frozen_steps, history, model_in, model_in_dtype};
  return launch_step("tg_step_epilogue", p, DdimUpdate{prediction_type}, advance, stream);
}

extern "C" int tg_step_epilogue_sigma(const float* noise_pred, float* latents, int32_t n_img, int32_t chw, int32_t hw,
                                      int32_t has_cfg, float guidance_scale, const float* coef, int32_t* step_idx, int32_t advance,
                                      const void* noise, int32_t noise_dtype, const float* frozen, const float* frozen_mask,
                                      int32_t mask_per_img, int32_t frozen_steps, float* history, void* model_in,
                                      int32_t model_in_dtype, void* stream) {
  TG_CHECK(!noise || src_dtype_ok(noise_dtype), TG_ERR_ARG, "tg_step_epilogue_sigma: noise dtype must be TG_BF16, TG_F16 or 2 (fp32)");
  TG_CHECK(!model_in || src_dtype_ok(model_in_dtype), TG_ERR_ARG, "tg_step_epilogue_sigma: model_in dtype must be TG_BF16, TG_F16 or 2 (fp32)");
  const StepCommon p{noise_pred, latents, n_img, chw, hw, has_cfg, guidance_scale, coef, step_idx, frozen,
                     frozen_mask, mask_per_img, frozen_steps, history, model_in, model_in_dtype};
  return launch_step("tg_step_epilogue_sigma", p, SigmaUpdate{noise, noise_dtype}, advance, stream);
}

extern "C" int tg_step_epilogue_dpm(const float* noise_pred, float* latents, float* x0_prev, int32_t n_img, int32_t chw, int32_t hw,
                                    int32_t has_cfg, float guidance_scale, const float* coef, int32_t* step_idx, int32_t advance,
                                    const float* frozen, const float* frozen_mask, int32_t mask_per_img, int32_t frozen_steps,
                                    float* history, void* model_in, int32_t model_in_dtype, void* stream) {
  TG_CHECK(x0_prev, TG_ERR_ARG, "tg_step_epilogue_dpm: bad args");
  TG_CHECK(x0_prev != latents && (const float*)x0_prev != noise_pred, TG_ERR_ARG, "tg_step_epilogue_dpm: x0_prev must be a buffer of its own");
  TG_CHECK(!model_in || src_dtype_ok(model_in_dtype), TG_ERR_ARG, "tg_step_epilogue_dpm: model_in dtype must be TG_BF16, TG_F16 or 2 (fp32)");
  const StepCommon p{noise_pred, latents, n_img, chw, hw, has_cfg, guidance_scale, coef, step_idx, frozen,
                     frozen_mask, mask_per_img, frozen_steps, history, model_in, model_in_dtype};
  return launch_step("tg_step_epilogue_dpm", p, DpmUpdate{x0_prev}, advance, stream);
}
