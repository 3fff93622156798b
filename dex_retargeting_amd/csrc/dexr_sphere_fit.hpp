// dexr_sphere_fit.hpp -- greedy inner-sphere cover of sampled signed-distance fields (include/dexr_sphere_fit.h): a fragment of
// dexr_pose.hip, which includes it once, before the mesh sampler.  It shares nothing with the robot kernels or the mesh kernels but
// DevBuf / POSE_HIP, finite_d and the error channel: it fits grids from any source.
//
// fit_init_kernel   one block per body: a thread owns rows (ix, iy) and builds the row's mask word, m per sample (-1: no candidate),
//                   the interior count; it also clears the body's outputs and evaluates the stop rule before round 0.
// fit_gain_kernel   blocks (chunk, body), FIT_THREADS threads, thread t of chunk c owns the samples c * CHUNK + j * FIT_THREADS + t:
//                   consecutive lanes hold consecutive iz of one row, so that with equal m they read the same LDS word at the same
//                   time (a broadcast); the mask is 64-bit words read with 64-bit loads.  The reduction to the block's best key is
//                   a shuffle tree per wave and one LDS step across the four waves.
// fit_apply_kernel  one block per body: reduces the body's slots the same way, then every thread clears the winner's interval from
//                   the rows it owns (a row belongs to one thread: plain stores).
//
// A key is two words compared in order: hi = gain << 32 | m and lo = ~index, so that the largest key is the rule of the header.
#include "dexr_sphere_fit.h"

#define FIT_THREADS 256
#define FIT_WAVES (FIT_THREADS / 64)
#define FIT_MAX_ROWS (DEXR_SPHERE_FIT_MAX_DIM * DEXR_SPHERE_FIT_MAX_DIM)
#define FIT_MAX_SAMPLES (FIT_MAX_ROWS * DEXR_SPHERE_FIT_MAX_DIM)
#define FIT_MAX_CHUNKS ((FIT_MAX_SAMPLES + DEXR_SPHERE_FIT_CHUNK - 1) / DEXR_SPHERE_FIT_CHUNK)
#define FIT_M_MAX 2147483647

static_assert(DEXR_SPHERE_FIT_MAX_DIM == 64, "a row of samples along z is one 64-bit word");
static_assert(DEXR_SPHERE_FIT_CHUNK % FIT_THREADS == 0 && FIT_THREADS % 64 == 0, "a thread owns a whole number of samples, a block whole waves");
static_assert(DEXR_SPHERE_FIT_MAX_BODIES * 32 <= 3072, "the body table travels as a kernel argument");
static_assert(DEXR_SPHERE_MAX <= 255 && DEXR_SPHERE_FIT_MAX_DIM <= 255, "a body's dimensions and sphere count are bytes of the table");

namespace {

struct FitBody {
  int64_t v_off;     // first sample in `values`
  double h;          // spacing
  int32_t mask_off;  // first word of the body's mask in the workspace's mask array
  int32_t m_off;     // first entry of the body's m in the workspace's m array
  uint8_t nx, ny, nz, k;
  uint8_t pad[4];
};
static_assert(sizeof(FitBody) == 32, "FitBody is 32 bytes");

struct FitJob {
  FitBody body[DEXR_SPHERE_FIT_MAX_BODIES];
  const float* values;
  uint64_t* mask;     // workspace: the masks of all bodies
  int32_t* m;         // workspace: m of every sample of every body, -1 where the sample is no candidate
  uint64_t* slot_hi;  // workspace: (n_body, FIT_MAX_CHUNKS) keys of the gain kernel's blocks
  uint32_t* slot_lo;
  int32_t* stop;      // workspace: (n_body)
  int32_t *index_out, *gain_out, *count_out;
  double min_radius, inflate, coverage;
  int32_t k_max;
};

struct FitKey {
  uint64_t hi;
  uint32_t lo;
};

__device__ __forceinline__ bool fit_less(const FitKey& a, const FitKey& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// floor(sqrt(x)), exact: the float root is a first guess, the comparisons decide (x < 2^31, so that (r + 1)^2 fits 32 unsigned bits)
__device__ __forceinline__ int32_t fit_isqrt(int32_t x) {
  uint32_t r = (uint32_t)sqrtf((float)x);
  const uint32_t ux = (uint32_t)x;
  while (r * r > ux) --r;
  while ((r + 1) * (r + 1) <= ux) ++r;
  return (int32_t)r;
}

// the bits iz - w .. iz + w of a row, clipped to 0 .. nz - 1, for w = isqrt(rem), rem >= 0
__device__ __forceinline__ uint64_t fit_interval(int32_t rem, int32_t iz, int32_t nz) {
  const int32_t w = fit_isqrt(rem);
  const int32_t lo = iz - w > 0 ? iz - w : 0, hi = iz + w < nz - 1 ? iz + w : nz - 1;
  return (~0ull >> (63 - (hi - lo))) << lo;
}

// the block's largest key, valid in thread 0; every thread of the block calls it
__device__ __forceinline__ FitKey fit_block_max(FitKey key, FitKey* across) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    FitKey o;
    o.hi = __shfl_down(key.hi, d, 64);
    o.lo = __shfl_down(key.lo, d, 64);
    if (fit_less(key, o)) key = o;
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) across[tid >> 6] = key;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < FIT_WAVES; ++w)
      if (fit_less(key, across[w])) key = across[w];
  return key;
}

__global__ void __launch_bounds__(FIT_THREADS) fit_init_kernel(FitJob J) {
  __shared__ int32_t part[FIT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const FitBody B = J.body[b];
  const int nx = B.nx, ny = B.ny, nz = B.nz;
  const float* v = J.values + B.v_off;
  uint64_t* mask = J.mask + B.mask_off;
  int32_t* m = J.m + B.m_off;
  int32_t interior = 0;
  for (int row = tid; row < nx * ny; row += FIT_THREADS) {
    uint64_t word = 0;
    for (int iz = 0; iz < nz; ++iz) {
      const float s = v[row * nz + iz];
      int32_t mm = -1;
      if (s < 0.f) {  // (a NaN fails the comparison)
        word |= 1ull << iz;
        const double r = (double)(-s);
        if (r >= J.min_radius) {
#pragma clang fp contract(off)
          const double t = (r + J.inflate) / B.h;
          const double q = floor(t * t);
          mm = q >= (double)FIT_M_MAX ? FIT_M_MAX : (int32_t)q;
        }
      }
      m[row * nz + iz] = mm;
    }
    mask[row] = word;
    interior += __popcll(word);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) interior += __shfl_down(interior, d, 64);
  if ((tid & 63) == 0) part[tid >> 6] = interior;
  for (int s = tid; s < J.k_max; s += FIT_THREADS) {
    J.index_out[b * J.k_max + s] = -1;
    J.gain_out[b * J.k_max + s] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    int32_t n = 0;
    for (int w = 0; w < FIT_WAVES; ++w) n += part[w];
    J.count_out[3 * b + 0] = n;
    J.count_out[3 * b + 1] = 0;
    J.count_out[3 * b + 2] = 0;
    J.stop[b] = 0.0 >= ceil(J.coverage * (double)n) ? 1 : 0;
  }
}

__global__ void __launch_bounds__(FIT_THREADS) fit_gain_kernel(FitJob J) {
  __shared__ uint64_t mask[FIT_MAX_ROWS];
  __shared__ FitKey across[FIT_WAVES];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (J.stop[b]) return;  // (uniform over the block)
  const FitBody B = J.body[b];
  const int nx = B.nx, ny = B.ny, nz = B.nz, n = nx * ny * nz;
  const int first = blockIdx.x * DEXR_SPHERE_FIT_CHUNK;
  if (first >= n) return;
  const uint64_t* gmask = J.mask + B.mask_off;
  for (int r = tid; r < nx * ny; r += FIT_THREADS) mask[r] = gmask[r];
  __syncthreads();
  const int32_t* m = J.m + B.m_off;
  FitKey best = {0ull, 0u};
  for (int j = 0; j < DEXR_SPHERE_FIT_CHUNK / FIT_THREADS; ++j) {
    const int s = first + j * FIT_THREADS + tid;
    if (s >= n) break;
    const int32_t mm = m[s];
    if (mm < 0) continue;
    const int ix = s / (ny * nz), r = s - ix * (ny * nz), iy = r / nz, iz = r - iy * nz;
    const int32_t reach = fit_isqrt(mm);
    const int x0 = ix - reach > 0 ? ix - reach : 0, x1 = ix + reach < nx - 1 ? ix + reach : nx - 1;
    int32_t gain = 0;
    for (int x = x0; x <= x1; ++x) {
      const int32_t rem_x = mm - (x - ix) * (x - ix);
      const int32_t ry = fit_isqrt(rem_x);
      const int y0 = iy - ry > 0 ? iy - ry : 0, y1 = iy + ry < ny - 1 ? iy + ry : ny - 1;
      for (int y = y0; y <= y1; ++y) gain += __popcll(mask[x * ny + y] & fit_interval(rem_x - (y - iy) * (y - iy), iz, nz));
    }
    const FitKey key = {((uint64_t)(uint32_t)gain << 32) | (uint32_t)mm, ~(uint32_t)s};
    if (fit_less(best, key)) best = key;
  }
  best = fit_block_max(best, across);
  if (tid == 0) {
    J.slot_hi[b * FIT_MAX_CHUNKS + blockIdx.x] = best.hi;
    J.slot_lo[b * FIT_MAX_CHUNKS + blockIdx.x] = best.lo;
  }
}

__global__ void __launch_bounds__(FIT_THREADS) fit_apply_kernel(FitJob J) {
  __shared__ FitKey across[FIT_WAVES];
  __shared__ FitKey winner;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (J.stop[b]) return;
  const FitBody B = J.body[b];
  const int nx = B.nx, ny = B.ny, nz = B.nz, n = nx * ny * nz;
  const int chunks = (n + DEXR_SPHERE_FIT_CHUNK - 1) / DEXR_SPHERE_FIT_CHUNK;
  FitKey best = {0ull, 0u};
  for (int c = tid; c < chunks; c += FIT_THREADS) {
    const FitKey key = {J.slot_hi[b * FIT_MAX_CHUNKS + c], J.slot_lo[b * FIT_MAX_CHUNKS + c]};
    if (fit_less(best, key)) best = key;
  }
  best = fit_block_max(best, across);
  if (tid == 0) winner = best;
  __syncthreads();
  best = winner;
  const int32_t gain = (int32_t)(best.hi >> 32), mm = (int32_t)(uint32_t)best.hi;
  if (gain == 0) {  // (uniform: nothing left that a candidate covers)
    if (tid == 0) J.stop[b] = 1;
    return;
  }
  const int s = (int)~best.lo;
  const int ix = s / (ny * nz), r = s - ix * (ny * nz), iy = r / nz, iz = r - iy * nz;
  uint64_t* gmask = J.mask + B.mask_off;
  for (int row = tid; row < nx * ny; row += FIT_THREADS) {
    const int x = row / ny, y = row - x * ny;
    const int32_t d2 = (x - ix) * (x - ix) + (y - iy) * (y - iy);
    if (d2 <= mm) gmask[row] &= ~fit_interval(mm - d2, iz, nz);
  }
  if (tid == 0) {
    const int32_t n_int = J.count_out[3 * b + 0], n_cov = J.count_out[3 * b + 1] + gain, n_sph = J.count_out[3 * b + 2];
    J.index_out[b * J.k_max + n_sph] = s;
    J.gain_out[b * J.k_max + n_sph] = gain;
    J.count_out[3 * b + 1] = n_cov;
    J.count_out[3 * b + 2] = n_sph + 1;
    if (n_sph + 1 >= (int32_t)B.k || (double)n_cov >= ceil(J.coverage * (double)n_int)) J.stop[b] = 1;
  }
}

// the parts of the workspace, in bytes from its start, each 16-byte aligned
struct FitLayout {
  size_t slot_hi, slot_lo, mask, m, stop, total;
};

size_t fit_align16(size_t n) { return (n + 15) & ~(size_t)15; }

// < 0 error; fills the layout and the table's offsets (table may be NULL)
int fit_layout(int32_t n_body, const int32_t* dims, FitLayout* L, FitBody* table) {
  if (n_body < 1 || n_body > DEXR_SPHERE_FIT_MAX_BODIES)
    return dexr_set_error(DEXR_ERR_INVALID, "a call fits 1..%d bodies, got %d", DEXR_SPHERE_FIT_MAX_BODIES, n_body);
  if (!dims) return dexr_set_error(DEXR_ERR_INVALID, "dims is NULL");
  size_t rows = 0, samples = 0;
  for (int b = 0; b < n_body; ++b) {
    for (int a = 0; a < 3; ++a)
      if (dims[3 * b + a] < DEXR_SPHERE_FIT_MIN_DIM || dims[3 * b + a] > DEXR_SPHERE_FIT_MAX_DIM)
        return dexr_set_error(DEXR_ERR_INVALID, "body %d: grid dimension %d is %d (%d..%d)", b, a, dims[3 * b + a], DEXR_SPHERE_FIT_MIN_DIM,
                              DEXR_SPHERE_FIT_MAX_DIM);
    if (table) {
      table[b].mask_off = (int32_t)rows;
      table[b].m_off = (int32_t)samples;
      table[b].nx = (uint8_t)dims[3 * b], table[b].ny = (uint8_t)dims[3 * b + 1], table[b].nz = (uint8_t)dims[3 * b + 2];
    }
    rows += (size_t)dims[3 * b] * dims[3 * b + 1];
    samples += (size_t)dims[3 * b] * dims[3 * b + 1] * dims[3 * b + 2];
  }
  L->slot_hi = 0;
  L->slot_lo = L->slot_hi + fit_align16((size_t)n_body * FIT_MAX_CHUNKS * sizeof(uint64_t));
  L->mask = L->slot_lo + fit_align16((size_t)n_body * FIT_MAX_CHUNKS * sizeof(uint32_t));
  L->m = L->mask + fit_align16(rows * sizeof(uint64_t));
  L->stop = L->m + fit_align16(samples * sizeof(int32_t));
  L->total = L->stop + fit_align16((size_t)n_body * sizeof(int32_t));
  return 0;
}

// every rule of the header but the pointers of the caller's side; fills the job but its device pointers
int fit_check(int32_t n_body, const int32_t* dims, const double* spacing, const int64_t* offset, const int32_t* k, double min_radius, double inflate,
              double coverage, int64_t n_values, FitJob* J, FitLayout* L) {
  memset(J, 0, sizeof(*J));
  const int c = fit_layout(n_body, dims, L, J->body);
  if (c) return c;
  if (!spacing || !offset || !k) return dexr_set_error(DEXR_ERR_INVALID, "spacing, offset or k is NULL");
  if (n_values < 0) return dexr_set_error(DEXR_ERR_INVALID, "negative value count");
  J->k_max = 0;
  for (int b = 0; b < n_body; ++b) {
    if (!finite_d(spacing[b]) || !(spacing[b] > 0.0)) return dexr_set_error(DEXR_ERR_INVALID, "body %d: spacing must be finite and > 0, got %g", b, spacing[b]);
    const int64_t n = (int64_t)dims[3 * b] * dims[3 * b + 1] * dims[3 * b + 2];
    if (offset[b] < 0 || offset[b] > n_values - n)
      return dexr_set_error(DEXR_ERR_INVALID, "body %d: samples %lld .. %lld lie outside the %lld values", b, (long long)offset[b], (long long)(offset[b] + n - 1),
                            (long long)n_values);
    if (k[b] < 1 || k[b] > DEXR_SPHERE_MAX) return dexr_set_error(DEXR_ERR_INVALID, "body %d: a body takes 1..%d spheres, got %d", b, DEXR_SPHERE_MAX, k[b]);
    J->body[b].v_off = offset[b];
    J->body[b].h = spacing[b];
    J->body[b].k = (uint8_t)k[b];
    if (k[b] > J->k_max) J->k_max = k[b];
  }
  if (!finite_d(min_radius) || !(min_radius >= 0.0)) return dexr_set_error(DEXR_ERR_INVALID, "min_radius must be finite and >= 0, got %g", min_radius);
  if (!finite_d(inflate) || !(inflate >= 0.0)) return dexr_set_error(DEXR_ERR_INVALID, "inflate must be finite and >= 0, got %g", inflate);
  if (!(coverage >= 0.0 && coverage <= 1.0)) return dexr_set_error(DEXR_ERR_INVALID, "coverage must lie in 0..1, got %g", coverage);
  J->min_radius = min_radius;
  J->inflate = inflate;
  J->coverage = coverage;
  return 0;
}

// the launches of one call: the first kernel, then two per round for the largest sphere count
int fit_launch(int32_t n_body, const int32_t* dims, FitJob& J, const FitLayout& L, const float* values, int32_t* index_out, int32_t* gain_out,
               int32_t* count_out, void* workspace, hipStream_t st) {
  char* ws = (char*)workspace;
  J.values = values;
  J.slot_hi = (uint64_t*)(ws + L.slot_hi);
  J.slot_lo = (uint32_t*)(ws + L.slot_lo);
  J.mask = (uint64_t*)(ws + L.mask);
  J.m = (int32_t*)(ws + L.m);
  J.stop = (int32_t*)(ws + L.stop);
  J.index_out = index_out;
  J.gain_out = gain_out;
  J.count_out = count_out;
  int chunks = 1;
  for (int b = 0; b < n_body; ++b) {
    const int n = dims[3 * b] * dims[3 * b + 1] * dims[3 * b + 2];
    chunks = std::max(chunks, (n + DEXR_SPHERE_FIT_CHUNK - 1) / DEXR_SPHERE_FIT_CHUNK);
  }
  hipLaunchKernelGGL(fit_init_kernel, dim3((unsigned)n_body), dim3(FIT_THREADS), 0, st, J);
  for (int round = 0; round < J.k_max; ++round) {
    hipLaunchKernelGGL(fit_gain_kernel, dim3((unsigned)chunks, (unsigned)n_body), dim3(FIT_THREADS), 0, st, J);
    hipLaunchKernelGGL(fit_apply_kernel, dim3((unsigned)n_body), dim3(FIT_THREADS), 0, st, J);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "sphere fit kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

}  // namespace

extern "C" {

size_t dexr_sphere_fit_workspace_bytes(int32_t n_body, const int32_t* dims) {
  FitLayout L;
  return fit_layout(n_body, dims, &L, nullptr) ? 0 : L.total;
}

int dexr_sphere_fit_dev(int32_t n_body, const int32_t* dims, const double* spacing, const int64_t* offset, const int32_t* k, double min_radius,
                        double inflate, double coverage, int64_t n_values, const float* values, int32_t* index_out, int32_t* gain_out,
                        int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream) {
  FitJob J;
  FitLayout L;
  const int c = fit_check(n_body, dims, spacing, offset, k, min_radius, inflate, coverage, n_values, &J, &L);
  if (c) return c;
  if (!values || !index_out || !gain_out || !count_out || !workspace) return dexr_set_error(DEXR_ERR_INVALID, "null values, output or workspace pointer");
  if (workspace_bytes < L.total) return dexr_set_error(DEXR_ERR_INVALID, "workspace of %zu B, %zu B needed", workspace_bytes, L.total);
  if ((uintptr_t)workspace & 15) return dexr_set_error(DEXR_ERR_INVALID, "the workspace must be 16-byte aligned");
  return fit_launch(n_body, dims, J, L, values, index_out, gain_out, count_out, workspace, (hipStream_t)stream);
}

int dexr_sphere_fit(int32_t n_body, const int32_t* dims, const double* spacing, const int64_t* offset, const int32_t* k, double min_radius,
                    double inflate, double coverage, int64_t n_values, const float* values, int32_t* index_out, int32_t* gain_out,
                    int32_t* count_out) {
  FitJob J;
  FitLayout L;
  const int c = fit_check(n_body, dims, spacing, offset, k, min_radius, inflate, coverage, n_values, &J, &L);
  if (c) return c;
  if (!values || !index_out || !gain_out || !count_out) return dexr_set_error(DEXR_ERR_INVALID, "null values or output pointer");
  const size_t n_out = (size_t)n_body * J.k_max * sizeof(int32_t), n_cnt = (size_t)n_body * 3 * sizeof(int32_t);
  DevBuf dv, di, dg, dc, dw;
  POSE_HIP(dv.put(values, (size_t)n_values * sizeof(float)));
  POSE_HIP(di.put(nullptr, n_out));
  POSE_HIP(dg.put(nullptr, n_out));
  POSE_HIP(dc.put(nullptr, n_cnt));
  POSE_HIP(dw.put(nullptr, L.total));
  const int rc = fit_launch(n_body, dims, J, L, (const float*)dv.p, (int32_t*)di.p, (int32_t*)dg.p, (int32_t*)dc.p, dw.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  POSE_HIP(hipMemcpy(index_out, di.p, n_out, hipMemcpyDeviceToHost));
  POSE_HIP(hipMemcpy(gain_out, dg.p, n_out, hipMemcpyDeviceToHost));
  POSE_HIP(hipMemcpy(count_out, dc.p, n_cnt, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

}  // extern "C"
