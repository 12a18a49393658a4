// Predicted perspective fields against ground truth: per-pixel errors, per-image statistics with an exact median, running histogram
// (include/pf_hip.h pf_field_errors).  Memory bound, no MFMA.
//   ferr_accum_kernel      grid (blocks per image) x (images), 256 threads: 16-byte loads of the six planes, the error maps written once,
//                          fp64 sums / max / counts per block -> one partial record per block (no float atomics), and the histogram of bits
//                          30..20 of both errors' patterns in LDS, added to the image's histogram with integer atomics (integer sums
//                          commute: the result is the same on every run)
//   ferr_pick_kernel<L>    one wave per image: (L = 0) partial records summed in block order in fp64 -> the output row but its medians;
//                          then for each of the four selections (ranks (n - 1) / 2 and n / 2 of e_up and of e_lat) the bucket of level L
//                          that holds the rank, appended to the selection's prefix; (L = 2) the 31 bits are complete -> medians
//   ferr_level_kernel<L>   L = 1, 2: rereads the error maps (8 B per pixel) and histograms the next digit (bits 19..9, then 8..0) of the
//                          elements that share a selection's prefix
//   ferr_dhist_kernel      optional: the maps binned at 1/64 degree in LDS, added to the caller's running int64 histogram
//   ferr_sums_kernel       optional: the group's per-image totals added to the caller's running totals in image order
// The errors are non-negative floats, so their bit patterns order like unsigned integers and bit 31 is always 0.
#include <math.h>

#include <algorithm>

#include "../../include/pf_hip.h"
#include "field_err.h"
#include "pf_kernels.h"

namespace pf {

namespace {

// partial record of one accumulate block: the valid pixels, then per metric sum, sum of squares, max, count below the threshold
enum : int { R_N = 0, R_SUM = 1, R_SQ = 2, R_MAX = 3, R_BELOW = 4, R_METRIC = 4, R_NV = 9 };
static_assert(R_NV <= FERR_REC, "record too small");
constexpr int kLevels = 3;
constexpr int kDigitBits[kLevels] = {11, 11, 9};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// 4 consecutive floats of a plane from element p0: one 16-byte load, or element by element with NaN beyond the end
__device__ __forceinline__ void load4(const float* p, long p0, long n, bool vec, float* v) {
  if (vec) {
    const float4 a = *reinterpret_cast<const float4*>(p + p0);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p0 + k < n ? p[p0 + k] : NAN;
  }
}
__device__ __forceinline__ void store4(float* p, long p0, long n, bool vec, const float* v) {
  if (vec) {
    *reinterpret_cast<float4*>(p + p0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (p0 + k < n) p[p0 + k] = v[k];
  }
}

// blocks per image of the level kernels: a quarter of the accumulate pass's.  Their digits spread over the whole LDS histogram, so every
// block flushes most of its bins with one global atomic each; fewer, longer blocks cut those (measured: DESIGN.md section 13)
__host__ __device__ __forceinline__ int ferr_level_blocks(int nblk) { return (nblk + 3) / 4; }

// the block's LDS histogram added to the image's: only the bins that were hit
__device__ __forceinline__ void flush_hist(const unsigned* lds, unsigned* g, int bins, int tid) {
  for (int k = tid; k < bins; k += 256) {
    const unsigned v = lds[k];
    if (v) atomicAdd(g + k, v);
  }
}

}  // namespace

// ---------------------------------------------------------------- accumulate: grid (blocks per image) x (images), 256 threads
__global__ __launch_bounds__(256) void ferr_accum_kernel(const FerrBatch fb) {
  const int img = blockIdx.y, tid = threadIdx.x;
  if (img >= fb.n || (int)blockIdx.x >= fb.nblk[img]) return;
  __shared__ unsigned hist[2 * FERR_LEVEL_BINS];
  for (int k = tid; k < 2 * FERR_LEVEL_BINS; k += 256) hist[k] = 0u;
  __syncthreads();
  const long n = (long)fb.H[img] * fb.W[img];
  const bool vec = fb.vec[img] != 0;
  const float* up_p = fb.up_pred[img];
  const float* up_g = fb.up_gt[img];
  const float* lat_p = fb.lat_pred[img];
  const float* lat_g = fb.lat_gt[img];
  float* err_up = fb.err_up[img];
  float* err_lat = fb.err_lat[img];
  const float thr = fb.threshold;
  double s_up = 0.0, q_up = 0.0, s_lat = 0.0, q_lat = 0.0;
  float m_up = 0.f, m_lat = 0.f;
  unsigned cnt = 0u, b_up = 0u, b_lat = 0u;
  const long nchunk = (n + 3) >> 2, stride = (long)fb.nblk[img] * 256;
  for (long q = (long)blockIdx.x * 256 + tid; q < nchunk; q += stride) {
    const long p0 = q << 2;
    float px[4], py[4], gx[4], gy[4], lp[4], lg[4], eu[4], el[4];
    load4(up_p, p0, n, vec, px);
    load4(up_p + n, p0, n, vec, py);
    load4(up_g, p0, n, vec, gx);
    load4(up_g + n, p0, n, vec, gy);
    load4(lat_p, p0, n, vec, lp);
    load4(lat_g, p0, n, vec, lg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const FieldErr e = field_error_at(px[k], py[k], gx[k], gy[k], lp[k], lg[k]);
      eu[k] = e.up;
      el[k] = e.lat;
      if (e.valid) {
        const double du = (double)e.up, dl = (double)e.lat;
        ++cnt;
        s_up += du;
        q_up = fma(du, du, q_up);
        s_lat += dl;
        q_lat = fma(dl, dl, q_lat);
        m_up = fmaxf(m_up, e.up);
        m_lat = fmaxf(m_lat, e.lat);
        b_up += e.up < thr ? 1u : 0u;
        b_lat += e.lat < thr ? 1u : 0u;
        atomicAdd(&hist[(__float_as_uint(e.up) >> 20) & (FERR_LEVEL_BINS - 1)], 1u);
        atomicAdd(&hist[FERR_LEVEL_BINS + ((__float_as_uint(e.lat) >> 20) & (FERR_LEVEL_BINS - 1))], 1u);
      }
    }
    store4(err_up, p0, n, vec, eu);
    store4(err_lat, p0, n, vec, el);
  }
  // wave reductions in fp64 (the counts are exact there), then the 4 waves in a fixed order
  __shared__ double red[4][R_NV];
  const int wave = tid >> 6, lane = tid & 63;
  double v[R_NV];
  v[R_N] = wave_sum((double)cnt);
  v[R_SUM] = wave_sum(s_up);
  v[R_SQ] = wave_sum(q_up);
  v[R_MAX] = wave_max((double)m_up);
  v[R_BELOW] = wave_sum((double)b_up);
  v[R_METRIC + R_SUM] = wave_sum(s_lat);
  v[R_METRIC + R_SQ] = wave_sum(q_lat);
  v[R_METRIC + R_MAX] = wave_max((double)m_lat);
  v[R_METRIC + R_BELOW] = wave_sum((double)b_lat);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < R_NV; ++k) red[wave][k] = v[k];
  }
  __syncthreads();  // also: every LDS histogram update of the block is done
  if (tid < R_NV) {
    double* part = fb.part[img] + (long)blockIdx.x * FERR_REC;
    const bool is_max = tid == R_MAX || tid == R_METRIC + R_MAX;
    part[tid] = is_max ? fmax(fmax(red[0][tid], red[1][tid]), fmax(red[2][tid], red[3][tid]))
                       : ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
  flush_hist(hist, fb.hist[img], 2 * FERR_LEVEL_BINS, tid);  // level 0: selections 0 (up) and 1 (lat)
}

// ---------------------------------------------------------------- next digit of the elements that share a selection's prefix
template <int LEVEL>
__global__ __launch_bounds__(256) void ferr_level_kernel(const FerrBatch fb) {
  constexpr int NB = 1 << kDigitBits[LEVEL];
  constexpr int DSHIFT = LEVEL == 1 ? kDigitBits[2] : 0, PSHIFT = DSHIFT + kDigitBits[LEVEL];
  const int img = blockIdx.y, tid = threadIdx.x;
  if (img >= fb.n) return;
  const int nblk = ferr_level_blocks(fb.nblk[img]);
  if ((int)blockIdx.x >= nblk) return;
  const FerrState* st = fb.state + img;
  if (st->sums[0][PF_FERR_SUM_N] == 0.0) return;
  __shared__ unsigned hist[FERR_SEL * NB];
  for (int k = tid; k < FERR_SEL * NB; k += 256) hist[k] = 0u;
  __syncthreads();
  const unsigned p0 = st->prefix[0], p1 = st->prefix[1], p2 = st->prefix[2], p3 = st->prefix[3];
  const long n = (long)fb.H[img] * fb.W[img];
  const bool vec = fb.vec[img] != 0;
  const float* err_up = fb.err_up[img];
  const float* err_lat = fb.err_lat[img];
  const long nchunk = (n + 3) >> 2, stride = (long)nblk * 256;
  for (long q = (long)blockIdx.x * 256 + tid; q < nchunk; q += stride) {
    float eu[4], el[4];
    load4(err_up, q << 2, n, vec, eu);
    load4(err_lat, q << 2, n, vec, el);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // an invalid pixel is NaN in both maps: its pattern is above every finite one and shares no selection's prefix
      const unsigned bu = __float_as_uint(eu[k]), bl = __float_as_uint(el[k]);
      const unsigned du = (bu >> DSHIFT) & (NB - 1), dl = (bl >> DSHIFT) & (NB - 1);
      if ((bu >> PSHIFT) == p0) atomicAdd(&hist[du], 1u);
      if ((bu >> PSHIFT) == p1) atomicAdd(&hist[NB + du], 1u);
      if ((bl >> PSHIFT) == p2) atomicAdd(&hist[2 * NB + dl], 1u);
      if ((bl >> PSHIFT) == p3) atomicAdd(&hist[3 * NB + dl], 1u);
    }
  }
  __syncthreads();
  unsigned* g = fb.hist[img] + (long)LEVEL * FERR_SEL * FERR_LEVEL_BINS;
#pragma unroll
  for (int j = 0; j < FERR_SEL; ++j) flush_hist(hist + j * NB, g + j * FERR_LEVEL_BINS, NB, tid);
}

// ---------------------------------------------------------------- pick: one wave per image
template <int LEVEL>
__global__ __launch_bounds__(64) void ferr_pick_kernel(const FerrBatch fb) {
  constexpr int NB = 1 << kDigitBits[LEVEL], PER = NB / 64;
  const int img = blockIdx.x, lane = threadIdx.x;
  if (img >= fb.n) return;
  FerrState* st = fb.state + img;
  double* out = fb.out + (long)img * PF_FERR_COLS;
  __shared__ double sum[R_NV];
  __shared__ unsigned val[FERR_SEL];
  if (LEVEL == 0) {
    if (lane < R_NV) {
      // 8 loads in flight, combined in block order
      const double* part = fb.part[img] + lane;
      const int nb = fb.nblk[img];
      const bool is_max = lane == R_MAX || lane == R_METRIC + R_MAX;
      double s = 0.0;
      for (int b0 = 0; b0 < nb; b0 += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = b0 + k < nb ? part[(long)(b0 + k) * FERR_REC] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s = is_max ? fmax(s, v[k]) : s + v[k];
      }
      sum[lane] = s;
    }
    __syncthreads();
    if (lane < 2) {  // lane = metric
      const double n = sum[R_N];
      const double* r = sum + lane * R_METRIC;
      double* o = out + lane * PF_FERR_COL_LAT_MEAN;
      st->sums[lane][PF_FERR_SUM_N] = n;
      st->sums[lane][PF_FERR_SUM_E] = r[R_SUM];
      st->sums[lane][PF_FERR_SUM_E2] = r[R_SQ];
      st->sums[lane][PF_FERR_SUM_MAX] = r[R_MAX];
      st->sums[lane][PF_FERR_SUM_BELOW] = r[R_BELOW];
      const bool any = n > 0.0;
      o[PF_FERR_COL_UP_MEAN] = any ? r[R_SUM] / n : (double)NAN;
      o[PF_FERR_COL_UP_MEDIAN] = (double)NAN;
      o[PF_FERR_COL_UP_RMSE] = any ? sqrt(r[R_SQ] / n) : (double)NAN;
      o[PF_FERR_COL_UP_MAX] = any ? r[R_MAX] : (double)NAN;
      o[PF_FERR_COL_UP_FRAC_BELOW] = any ? r[R_BELOW] / n : (double)NAN;
      if (lane == 0) out[PF_FERR_COL_VALID_PIXELS] = n;
    }
  }
  const unsigned long long n = (unsigned long long)(LEVEL == 0 ? sum[R_N] : st->sums[0][PF_FERR_SUM_N]);
  if (n == 0) return;  // the medians stay NaN
  const unsigned* h = fb.hist[img] + (long)LEVEL * FERR_SEL * FERR_LEVEL_BINS;
#pragma unroll
  for (int j = 0; j < FERR_SEL; ++j) {
    const unsigned long long rank = LEVEL == 0 ? ((j & 1) ? n / 2 : (n - 1) / 2) : st->rank[j];
    const unsigned prefix = LEVEL == 0 ? 0u : st->prefix[j];
    const unsigned* hj = h + (LEVEL == 0 ? (j >> 1) : j) * FERR_LEVEL_BINS + lane * PER;
    unsigned c[PER];
    unsigned long long t = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { c[k] = hj[k]; t += c[k]; }
    unsigned long long incl = t;  // inclusive scan over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const unsigned long long excl = incl - t;
    if (excl <= rank && rank < incl) {  // exactly one lane: the counts of a level add up to what the level above found
      unsigned long long r = rank - excl;
      int b = 0;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        if (b == k && r >= c[k]) { r -= c[k]; b = k + 1; }
      }
      const unsigned found = (prefix << kDigitBits[LEVEL]) | (unsigned)(lane * PER + b);
      st->rank[j] = r;
      st->prefix[j] = found;
      if (LEVEL == kLevels - 1) val[j] = found;
    }
  }
  if (LEVEL == kLevels - 1) {
    __syncthreads();
    if (lane < 2)  // numpy's median: the mean of the two middle elements, in fp64 (the same element twice for an odd n)
      out[lane * PF_FERR_COL_LAT_MEAN + PF_FERR_COL_UP_MEDIAN] = 0.5 * ((double)__uint_as_float(val[2 * lane]) + (double)__uint_as_float(val[2 * lane + 1]));
  }
}

// ---------------------------------------------------------------- running histogram: grid (blocks per image) x (images) x (metric)
__global__ __launch_bounds__(256) void ferr_dhist_kernel(const FerrBatch fb, unsigned long long* d_hist) {
  const int img = blockIdx.y, metric = blockIdx.z, tid = threadIdx.x;
  if (img >= fb.n) return;
  const int nblk = ferr_level_blocks(fb.nblk[img]);
  if ((int)blockIdx.x >= nblk) return;
  __shared__ unsigned hist[PF_FERR_BINS];
  for (int k = tid; k < PF_FERR_BINS; k += 256) hist[k] = 0u;
  __syncthreads();
  const long n = (long)fb.H[img] * fb.W[img];
  const bool vec = fb.vec[img] != 0;
  const float* err = metric == 0 ? fb.err_up[img] : fb.err_lat[img];
  const long nchunk = (n + 3) >> 2, stride = (long)nblk * 256;
  for (long q = (long)blockIdx.x * 256 + tid; q < nchunk; q += stride) {
    float e[4];
    load4(err, q << 2, n, vec, e);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e[k] == e[k]) atomicAdd(&hist[(int)fminf(e[k] * (float)PF_FERR_BINS_PER_DEG, (float)(PF_FERR_BINS - 1))], 1u);
  }
  __syncthreads();
  unsigned long long* g = d_hist + (long)metric * PF_FERR_BINS;
  for (int k = tid; k < PF_FERR_BINS; k += 256) {
    const unsigned v = hist[k];
    if (v) atomicAdd(g + k, (unsigned long long)v);
  }
}

// the group's per-image totals added to the running totals, in image order
__global__ __launch_bounds__(64) void ferr_sums_kernel(const FerrBatch fb, double* d_sums) {
  const int lane = threadIdx.x;
  if (lane >= 2 * PF_FERR_SUMS) return;
  const int metric = lane / PF_FERR_SUMS, col = lane % PF_FERR_SUMS;
  double s = d_sums[lane];
  for (int i = 0; i < fb.n; ++i) {
    const double v = fb.state[i].sums[metric][col];
    s = col == PF_FERR_SUM_MAX ? fmax(s, v) : s + v;
  }
  d_sums[lane] = s;
}

int ferr_blocks_per_image(int H, int W) {
  const long n = (long)H * W;
  return (int)std::min<long>(std::max<long>((n + 4095) / 4096, 1), 256);
}

void launch_field_errors(const FerrBatch& fb, hipStream_t s) {
  int mx = 1;
  for (int k = 0; k < fb.n; ++k) mx = std::max(mx, fb.nblk[k]);
  const dim3 grid(mx, fb.n);
  hipLaunchKernelGGL(ferr_accum_kernel, grid, dim3(256), 0, s, fb);
  hipLaunchKernelGGL(ferr_pick_kernel<0>, dim3(fb.n), dim3(64), 0, s, fb);
  const dim3 grid_level(ferr_level_blocks(mx), fb.n);
  hipLaunchKernelGGL(ferr_level_kernel<1>, grid_level, dim3(256), 0, s, fb);
  hipLaunchKernelGGL(ferr_pick_kernel<1>, dim3(fb.n), dim3(64), 0, s, fb);
  hipLaunchKernelGGL(ferr_level_kernel<2>, grid_level, dim3(256), 0, s, fb);
  hipLaunchKernelGGL(ferr_pick_kernel<2>, dim3(fb.n), dim3(64), 0, s, fb);
}

void launch_field_errors_hist(const FerrBatch& fb, long long* d_hist, double* d_hist_sums, hipStream_t s) {
  int mx = 1;
  for (int k = 0; k < fb.n; ++k) mx = std::max(mx, fb.nblk[k]);
  hipLaunchKernelGGL(ferr_dhist_kernel, dim3(ferr_level_blocks(mx), fb.n, 2), dim3(256), 0, s, fb, reinterpret_cast<unsigned long long*>(d_hist));
  hipLaunchKernelGGL(ferr_sums_kernel, dim3(1), dim3(64), 0, s, fb, d_hist_sums);
}

}  // namespace pf
