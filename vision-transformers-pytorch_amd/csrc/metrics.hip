// Loss and prec@k meters of the reference trainer (train.py:277-281, 335-386; train_util.py:34-67) on the device: what the
// reference computes per batch with topk / eq / sum / cross_entropy and three .item() calls is two launches and no
// host synchronisation here.
//
//   cls_metrics_kernel          one 256-thread workgroup per row of the (B, K) logits, the row read ONCE:
//                                 ce_rows[b] = logsumexp(row) - row[label]        (F.cross_entropy, reduction "none")
//                                 rank[b]    = #{j : x_j > x_l} + #{j < l : x_j == x_l}
//                               = the label's position in a STABLE descending sort (among equal logits the lower class index
//                               ranks first); the label is in the top k exactly when rank < k.  (torch.topk leaves the order
//                               of ties unspecified; this rule is the contract, include/vtx.h.)
//   cls_meter_accumulate_kernel one workgroup; adds the batch to a device meter of 2 + nk doubles
//                               [n, loss_sum, hits_k0, hits_k1, ...] in a fixed order (no atomics: two runs on the same
//                               inputs give the same bits; doubles hold the counts exactly).
//
// Rows start wherever b * K * sizeof(T) puts them (K = 257 in bf16: a 2-byte boundary that moves from row to row): the
// elements before the first 16-byte boundary and behind the last whole vector are read one by one, the rest as 16-byte
// vectors.  Row statistics are fp32 (online maximum / sum of exponentials, as mix_loss_kernel), reductions are wave
// shuffles followed by the 4 wave partials in index order.
#include "vtx_common.h"

struct ClsKs { int k[8]; };

template <typename T> struct MetVec;
template <> struct MetVec<bf16> {
  static constexpr int N = 8;
  bf16x8 v;
  __device__ __forceinline__ float get(int i) const { return (float)v[i]; }
};
template <> struct MetVec<float> {
  static constexpr int N = 4;
  f32x4 v;
  __device__ __forceinline__ float get(int i) const { return v[i]; }
};

// per-thread state of the sweep
struct MetStat {
  float m, l;          // online softmax over the non-NaN logits: maximum, sum of exp(x - m)
  int gt, eqb, nnan;   // logits ordered above the label's / equal to it at a lower index / NaN logits
};

// NE consecutive logits x[0..NE) = classes j0 .. j0 + NE - 1.  Order: NaN above +inf, NaNs equal to each other.
template <int NE>
__device__ __forceinline__ void met_chunk(MetStat& s, const float* x, int j0, float xl, bool xl_nan, int label) {
  float xs[NE];
  float cmax = -INFINITY;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const float xe = x[e];
    const bool isn = xe != xe;
    const bool above = !xl_nan && (isn || xe > xl);
    const bool same = xl_nan ? isn : (xe == xl);
    s.gt += above ? 1 : 0;
    s.eqb += (same && j0 + e < label) ? 1 : 0;
    s.nnan += isn ? 1 : 0;
    xs[e] = isn ? -INFINITY : xe;
    cmax = fmaxf(cmax, xs[e]);
  }
  const float M = fmaxf(s.m, cmax);
  if (M > -INFINITY) {               // (a chunk of -inf on an empty state changes nothing: no -inf - -inf)
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) a += __expf(xs[e] - M);      // exp(-inf) = 0
    s.l = s.l * __expf(s.m - M) + a;                          // s.m = -inf: 0 * 0
    s.m = M;
  }
}

__device__ __forceinline__ void met_combine(float& m, float& l, float m2, float l2) {
  const float M = fmaxf(m, m2);
  l = (m == -INFINITY ? 0.f : l * __expf(m - M)) + (m2 == -INFINITY ? 0.f : l2 * __expf(m2 - M));
  m = M;
}

__device__ __forceinline__ int met_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void cls_metrics_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels,
                                                         float* __restrict__ ce_rows, int32_t* __restrict__ rank, int K,
                                                         int64_t ignore_index) {
  constexpr int N = MetVec<T>::N;
  __shared__ float redf[8];
  __shared__ int redi[12];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t lab = labels[b];
  if (lab == ignore_index) {                       // not counted (block-uniform exits: nothing of the row is read)
    if (tid == 0) { ce_rows[b] = 0.f; rank[b] = -1; }
    return;
  }
  if (lab < 0 || lab >= (int64_t)K) {              // never an index; counted, and the NaN shows in the epoch's loss
    if (tid == 0) { ce_rows[b] = __builtin_nanf(""); rank[b] = K; }
    return;
  }
  const int label = (int)lab;
  const T* row = logits + (int64_t)b * K;
  const float xl = to_f32<T>(row[label]);
  const bool xl_nan = xl != xl;

  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / sizeof(T));   // elements before the 16-byte boundary
  if (head > K) head = K;
  const int nvec = (K - head) / N;
  const int tail0 = head + nvec * N;

  MetStat s = {-INFINITY, 0.f, 0, 0, 0};
  if (tid < head) {                                // head < N <= 8
    const float x = to_f32<T>(row[tid]);
    met_chunk<1>(s, &x, tid, xl, xl_nan, label);
  }
  if (tail0 + tid < K) {                           // K - tail0 < N
    const float x = to_f32<T>(row[tail0 + tid]);
    met_chunk<1>(s, &x, tail0 + tid, xl, xl_nan, label);
  }
  const MetVec<T>* vrow = reinterpret_cast<const MetVec<T>*>(row + head);
#pragma unroll 2
  for (int v = tid; v < nvec; v += 256) {
    const MetVec<T> q = vrow[v];
    float x[N];
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = q.get(e);
    met_chunk<N>(s, x, head + v * N, xl, xl_nan, label);
  }

#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float m2 = shfl_xor_f(s.m, o), l2 = shfl_xor_f(s.l, o);
    met_combine(s.m, s.l, m2, l2);
  }
  const int gt = met_wave_sum(s.gt), eqb = met_wave_sum(s.eqb), nnan = met_wave_sum(s.nnan);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) {
    redf[2 * wave] = s.m; redf[2 * wave + 1] = s.l;
    redi[3 * wave] = gt; redi[3 * wave + 1] = eqb; redi[3 * wave + 2] = nnan;
  }
  __syncthreads();
  if (tid == 0) {
    float m = redf[0], l = redf[1];
    int g = redi[0], q = redi[1], nn = redi[2];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      met_combine(m, l, redf[2 * w], redf[2 * w + 1]);
      g += redi[3 * w]; q += redi[3 * w + 1]; nn += redi[3 * w + 2];
    }
    float ce;
    if (nn > 0) ce = __builtin_nanf("");                             // a NaN logit: the row's cross entropy is NaN
    else if (m == INFINITY) ce = xl == INFINITY ? __builtin_nanf("") : INFINITY;    // as logsumexp - x_l
    else ce = (m - xl) + __logf(l);                                  // (label on the maximum: exactly log l)
    ce_rows[b] = ce;
    rank[b] = g + q;
  }
}

// meter[0] += counted rows, meter[1] += loss, meter[2 + i] += rows with rank < ks[i].  Thread t sums rows t, t + 256, ...
// in fp64, then a fixed tree over the 256 partials.
__global__ __launch_bounds__(256) void cls_meter_accumulate_kernel(const float* __restrict__ ce_rows,
                                                                  const int32_t* __restrict__ rank,
                                                                  double* __restrict__ meter, ClsKs ks, int nk,
                                                                  const float* __restrict__ loss_override,
                                                                  float loss_scale, int B) {
  __shared__ double red[10][256];
  const int tid = threadIdx.x;
  double n = 0.0, loss = 0.0;
  double hits[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = tid; b < B; b += 256) {
    const int r = rank[b];
    if (r < 0) continue;                           // ignored label
    n += 1.0;
    loss += (double)ce_rows[b];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nk && r < ks.k[i]) hits[i] += 1.0;
  }
  red[0][tid] = n; red[1][tid] = loss;
#pragma unroll
  for (int i = 0; i < 8; ++i) red[2 + i][tid] = hits[i];
  __syncthreads();
  for (int sft = 128; sft >= 1; sft >>= 1) {
    if (tid < sft) {
#pragma unroll
      for (int qn = 0; qn < 10; ++qn) red[qn][tid] += red[qn][tid + sft];
    }
    __syncthreads();
  }
  if (tid < 2 + nk) {
    double add = red[tid][0];
    if (tid == 1 && loss_override != nullptr) add = (double)loss_override[0] * (double)loss_scale * red[0][0];
    meter[tid] += add;
  }
}

extern "C" {

/* include/vtx.h: vtx_cls_metrics */
int vtx_cls_metrics(const void* logits, const int64_t* labels, float* ce_rows, int32_t* rank, double* meter,
                    const int32_t* ks, int nk, const float* loss_override, float loss_scale, int B, int K,
                    int64_t ignore_index, int dtype, void* stream) {
  if (!logits || !labels || !ce_rows || !rank) return VTX_ERR_NULL;
  if (B <= 0 || K <= 0 || nk < 0 || nk > 8) return VTX_ERR_SHAPE;
  if (nk > 0 && !ks) return VTX_ERR_NULL;
  if (dtype != VTX_BF16 && dtype != VTX_F32) return VTX_ERR_DTYPE;
  if ((uintptr_t)logits & (dtype == VTX_BF16 ? 1u : 3u)) return VTX_ERR_ALIGN;
  ClsKs kk;
  for (int i = 0; i < 8; ++i) {
    kk.k[i] = i < nk ? ks[i] : 0;
    if (i < nk && ks[i] < 1) return VTX_ERR_SHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VTX_BF16)
    hipLaunchKernelGGL((cls_metrics_kernel<bf16>), dim3(B), dim3(256), 0, st, (const bf16*)logits, labels, ce_rows, rank, K,
                       ignore_index);
  else
    hipLaunchKernelGGL((cls_metrics_kernel<float>), dim3(B), dim3(256), 0, st, (const float*)logits, labels, ce_rows, rank, K,
                       ignore_index);
  if (meter)
    hipLaunchKernelGGL(cls_meter_accumulate_kernel, dim3(1), dim3(256), 0, st, (const float*)ce_rows, (const int32_t*)rank,
                       meter, kk, nk, loss_override, loss_scale, B);
  return vtx_check_launch();
}

}  // extern "C"
