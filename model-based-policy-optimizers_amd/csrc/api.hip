// api.hip — library-level entry points and host-side argument validation shared by all kernels.
#include "common.hpp"
#include <atomic>
#include <stdlib.h>
#include <string.h>

static thread_local char g_err[512] = "";

void mbpo_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *mbpo_last_error(void) { return g_err; }

extern "C" int mbpo_version(void) { return 100; /* 0.1.0 */ }

int mbpo_make_mlp_dev(const mbpo_mlp_desc *d, MlpDev *out, const char *name) {
  MBPO_REQUIRE(d != nullptr, MBPO_ERR_ARG, "%s: null mlp descriptor", name);
  MBPO_REQUIRE(d->params != nullptr, MBPO_ERR_ARG, "%s: null params", name);
  MBPO_REQUIRE(d->n_layers >= 1 && d->n_layers <= MBPO_MAX_LAYERS, MBPO_ERR_ARG, "%s: n_layers=%d out of [1,%d]", name,
               d->n_layers, MBPO_MAX_LAYERS);
  MBPO_REQUIRE(d->n_nets >= 1, MBPO_ERR_ARG, "%s: n_nets=%d < 1", name, d->n_nets);
  MBPO_REQUIRE(d->activation >= 0 && d->activation <= 2, MBPO_ERR_ARG, "%s: unknown activation %d", name, d->activation);
  int off = 0;
  for (int l = 0; l <= d->n_layers; ++l) {
    MBPO_REQUIRE(d->dims[l] >= 1 && d->dims[l] <= 4096, MBPO_ERR_ARG, "%s: dims[%d]=%d out of range", name, l, d->dims[l]);
    out->dims[l] = d->dims[l];
  }
  for (int l = 0; l < d->n_layers; ++l) {
    out->w_off[l] = off;
    off += d->dims[l] * d->dims[l + 1];
    out->b_off[l] = off;
    off += d->dims[l + 1];
  }
  MBPO_REQUIRE(d->n_nets == 1 || d->net_stride >= off, MBPO_ERR_ARG, "%s: net_stride=%lld < params per net %d", name,
               (long long)d->net_stride, off);
  out->params = d->params;
  out->net_stride = d->net_stride;
  out->n_nets = d->n_nets;
  out->n_layers = d->n_layers;
  out->act = d->activation;
  out->n_params = off;
  return MBPO_OK;
}

int mbpo_make_mlp_dev_from(const int *dims, int n_layers, int activation, const float *params, int n_nets, const char *name,
                           MlpDev *out) {
  mbpo_mlp_desc md;
  md.params = params ? params : (const float *)16;      // placeholder for size queries
  md.net_stride = 0;
  md.n_nets = n_nets;
  md.n_layers = n_layers;
  for (int l = 0; l <= n_layers && l <= MBPO_MAX_LAYERS; ++l) md.dims[l] = dims[l];
  md.activation = activation;
  return mbpo_make_mlp_dev(&md, out, name);
}

int mbpo_num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}

// ---------------------------------------------------------------------------------------------- knobs (knobs.hpp)
namespace {
struct KnobDef {
  const char *env;
  long long dflt;
  bool reread;
};
const KnobDef g_knob_def[KNOB_COUNT] = {
#define MBPO_KNOB_DEF_(id, env, dflt, reread, meaning) {env, dflt, reread},
    MBPO_KNOB_TABLE(MBPO_KNOB_DEF_)
#undef MBPO_KNOB_DEF_
};
struct KnobState {
  std::atomic<bool> cached{false};
  std::atomic<long long> value{0};
  std::atomic<int> override_{-1};
};
KnobState g_knob[KNOB_COUNT];
}  // namespace

long long mbpo_knob(KnobId id) {
  const KnobDef &k = g_knob_def[id];
  KnobState &s = g_knob[id];
  // the environment is read on the first query even under an override (what a function-level static did before the table)
  long long v;
  if (!k.reread && s.cached.load(std::memory_order_acquire)) {
    v = s.value.load(std::memory_order_relaxed);
  } else {
    const char *e = k.env ? getenv(k.env) : nullptr;
    v = e ? atoll(e) : k.dflt;
    s.value.store(v, std::memory_order_relaxed);
    s.cached.store(true, std::memory_order_release);
  }
  const int o = s.override_.load(std::memory_order_relaxed);
  return o >= 0 ? o : v;
}

int mbpo_knob_override(KnobId id) { return g_knob[id].override_.load(std::memory_order_relaxed); }

int mbpo_knob_set_override(KnobId id, int mode) {
  g_knob[id].override_.store(mode, std::memory_order_relaxed);
  return MBPO_OK;
}

// ---------------------------------------------------------------------------------------------- device RNG control words
__global__ void k_rng_advance(unsigned long long *rng, unsigned long long inc) {
  if (threadIdx.x == 0 && blockIdx.x == 0) rng[1] += inc;
}

extern "C" int mbpo_rng_advance(uint64_t *rng_dev, uint64_t inc, void *stream) {
  MBPO_REQUIRE(rng_dev, MBPO_ERR_ARG, "rng_advance: null rng_dev");
  hipLaunchKernelGGL(k_rng_advance, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long *)rng_dev, (unsigned long long)inc);
  MBPO_CHECK_LAUNCH("rng_advance");
  return MBPO_OK;
}

// ---------------------------------------------------------------------------------------------- standard-normal fill
// out[i] = philox_normal(seed + rng_dev[0], offset + rng_dev[1], stream, elem_base + i): the draws a fused kernel makes in
// registers, as a tensor — for host-side loops that walk a horizon step by step with a user's code between the kernels (BPTT
// through a user-defined System) and must consume the SAME numbers as the fused kernel (k_bptt_actor: element (traj*H + t)*u + d).
__global__ void __launch_bounds__(256) k_philox_normal_fill(unsigned long long seed, unsigned long long offset, const unsigned long long *rng_dev,
                                                            unsigned int stream, unsigned long long elem_base, long long n, float *out) {
  const RngKey k = rng_resolve(seed, offset, rng_dev);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    out[i] = philox_normal(k.seed, k.offset, stream, elem_base + (unsigned long long)i);
}

extern "C" int mbpo_philox_normal_fill(uint64_t seed, uint64_t offset, const uint64_t *rng_dev, uint32_t stream, uint64_t elem_base,
                                       int64_t n, float *out, void *stream_) {
  MBPO_REQUIRE(out && n > 0, MBPO_ERR_ARG, "philox_normal_fill: null out / n <= 0");
  MBPO_REQUIRE(stream >= 1 && stream <= 10, MBPO_ERR_ARG, "philox_normal_fill: unknown stream id %u", stream);
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_philox_normal_fill, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream_,
                     (unsigned long long)seed, (unsigned long long)offset, (const unsigned long long *)rng_dev, stream,
                     (unsigned long long)elem_base, (long long)n, out);
  MBPO_CHECK_LAUNCH("philox_normal_fill");
  return MBPO_OK;
}

__global__ void __launch_bounds__(256) k_philox_randint_fill(unsigned long long seed, unsigned long long offset, const unsigned long long *rng_dev,
                                                             unsigned int stream, unsigned long long elem_base, long long n, int lo, int hi,
                                                             int *out) {
  const RngKey k = rng_resolve(seed, offset, rng_dev);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    out[i] = philox_randint(k.seed, k.offset, stream, elem_base + (unsigned long long)i, lo, hi);
}

extern "C" int mbpo_philox_randint_fill(uint64_t seed, uint64_t offset, const uint64_t *rng_dev, uint32_t stream, uint64_t elem_base,
                                        int64_t n, int32_t lo, int32_t hi, int32_t *out, void *stream_) {
  MBPO_REQUIRE(out && n > 0, MBPO_ERR_ARG, "philox_randint_fill: null out / n <= 0");
  MBPO_REQUIRE(stream >= 1 && stream <= 10, MBPO_ERR_ARG, "philox_randint_fill: unknown stream id %u", stream);
  MBPO_REQUIRE(hi > lo, MBPO_ERR_ARG, "philox_randint_fill: empty range [%d, %d)", lo, hi);
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_philox_randint_fill, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream_,
                     (unsigned long long)seed, (unsigned long long)offset, (const unsigned long long *)rng_dev, stream,
                     (unsigned long long)elem_base, (long long)n, (int)lo, (int)hi, (int *)out);
  MBPO_CHECK_LAUNCH("philox_randint_fill");
  return MBPO_OK;
}

// ---------------------------------------------------------------------------------------------- grouped fill (batched problems)
// out[(s B + b) G + j] = draw(seeds[b], offset, stream, s G + j): the numbers n_problems independent launches over G elements per
// step would draw, each under its own seed, laid out step-major over the problems — the [S][B G] layout of a batched rollout whose
// problem b owns envs [b G', (b+1) G').
template <bool INT>
__global__ void __launch_bounds__(256) k_philox_fill_grouped(const unsigned long long *seeds, unsigned long long offset, unsigned int stream,
                                                             long long n_problems, long long group, long long n, int lo, int hi,
                                                             void *out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long sb = i / group, j = i - sb * group, s = sb / n_problems, b = sb - s * n_problems;
    const unsigned long long idx = (unsigned long long)(s * group + j);
    if constexpr (INT) ((int *)out)[i] = philox_randint(seeds[b], offset, stream, idx, lo, hi);
    else ((float *)out)[i] = philox_normal(seeds[b], offset, stream, idx);
  }
}

extern "C" int mbpo_philox_fill_grouped(const uint64_t *seeds, uint64_t offset, uint32_t stream, int32_t n_steps, int32_t n_problems,
                                        int64_t group, int32_t as_int, int32_t lo, int32_t hi, void *out, void *stream_) {
  MBPO_REQUIRE(seeds, MBPO_ERR_ARG, "philox_fill_grouped: seeds is NULL");
  MBPO_REQUIRE(out, MBPO_ERR_ARG, "philox_fill_grouped: out is NULL");
  MBPO_REQUIRE(n_problems > 0, MBPO_ERR_ARG, "philox_fill_grouped: n_problems=%d <= 0", n_problems);
  MBPO_REQUIRE(n_steps > 0 && group > 0, MBPO_ERR_ARG, "philox_fill_grouped: n_steps=%d, group=%lld must be > 0", n_steps, (long long)group);
  MBPO_REQUIRE(stream >= 1 && stream <= 10, MBPO_ERR_ARG, "philox_fill_grouped: unknown stream id %u", stream);
  MBPO_REQUIRE(!as_int || hi > lo, MBPO_ERR_ARG, "philox_fill_grouped: empty range [%d, %d)", lo, hi);
  const long long n = (long long)n_steps * n_problems * group;
  const long long blocks = (n + 255) / 256;
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
  if (as_int)
    hipLaunchKernelGGL(k_philox_fill_grouped<true>, grid, dim3(256), 0, (hipStream_t)stream_, (const unsigned long long *)seeds,
                       (unsigned long long)offset, stream, (long long)n_problems, (long long)group, n, (int)lo, (int)hi, out);
  else
    hipLaunchKernelGGL(k_philox_fill_grouped<false>, grid, dim3(256), 0, (hipStream_t)stream_, (const unsigned long long *)seeds,
                       (unsigned long long)offset, stream, (long long)n_problems, (long long)group, n, 0, 0, out);
  MBPO_CHECK_LAUNCH("philox_fill_grouped");
  return MBPO_OK;
}

// Test hook (not part of include/mbpo_hip.h): y[i] = helper fn (x[i]) for the fast_math.hpp helpers the elementwise sections use —
// 0 fm_exp, 1 fm_log, 2 fm_softplus, 3 fm_tanh, 4 fm_atanh, 5 fast_sigmoid, 6 swish (act_apply), 7 swish' (act_grad),
// 8 fm_softplus_fast, 9 fm_tanh_fast.
// tests/test_gpu_fastmath.py sweeps each against fp64.
enum { FM_EXP, FM_LOG, FM_SOFTPLUS, FM_TANH, FM_ATANH, FM_SIGMOID, FM_SWISH, FM_SWISH_GRAD, FM_SOFTPLUS_FAST, FM_TANH_FAST, FM_N };
__global__ void __launch_bounds__(256) k_debug_eval_fastmath(int fn, const float *x, float *y, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = x[i];
    float r;
    switch (fn) {
      case FM_EXP: r = fm_exp(v); break;
      case FM_LOG: r = fm_log(v); break;
      case FM_SOFTPLUS: r = fm_softplus(v); break;
      case FM_TANH: r = fm_tanh(v); break;
      case FM_ATANH: r = fm_atanh(v); break;
      case FM_SIGMOID: r = fast_sigmoid(v); break;
      case FM_SWISH: r = act_apply(v, MBPO_ACT_SWISH); break;
      case FM_SWISH_GRAD: r = act_grad(v, MBPO_ACT_SWISH); break;
      case FM_SOFTPLUS_FAST: r = fm_softplus_fast(v); break;
      default: r = fm_tanh_fast(v); break;
    }
    y[i] = r;
  }
}

extern "C" int mbpo_debug_eval_fastmath(int fn, const float *x, float *y, int64_t n, void *stream) {
  MBPO_REQUIRE(fn >= 0 && fn < FM_N, MBPO_ERR_ARG, "debug_eval_fastmath: unknown helper fn=%d (0..%d)", fn, FM_N - 1);
  MBPO_REQUIRE(n >= 0, MBPO_ERR_ARG, "debug_eval_fastmath: n=%lld < 0", (long long)n);
  if (n == 0) return MBPO_OK;
  MBPO_REQUIRE(x && y, MBPO_ERR_ARG, "debug_eval_fastmath: null pointer");
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_debug_eval_fastmath, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, fn, x, y,
                     (long long)n);
  MBPO_CHECK_LAUNCH("debug_eval_fastmath");
  return MBPO_OK;
}
