// Non-dominated filter on gfx950: omb_nondominated.
//
// S independent point sets, minimisation; coordinate j of point i of set s is y[(j·S + s)·ld + i] (omb_paths_eval's
// layout).  a dominates b when a_j ≤ b_j for every j and a_j < b_j for some j, in IEEE comparisons: −0.0 equals +0.0,
// ±∞ are ordinary values and a point with a NaN dominates nobody.  mask[s·ldm + i] = 1 when no point of set s
// dominates i and no coordinate of i is NaN.
//
// A sieve.  The work is all-pairs in the worst case (an antichain keeps every point) and tiny in the usual one (2^20
// iid points in two dimensions keep about 14), so:
//   tile pass   a workgroup of kNdTile lanes holds kNdTile points of one set in LDS (point-major, K doubles each:
//               64 KiB at K = 8), every lane tests its own point against the tile — all lanes read the same LDS address
//               per step, a broadcast — and the survivors' indices are appended to a list.  The first pass runs over
//               the points themselves, drops the NaN rows and clears the mask bytes; later passes run over the list.
//   final pass  every remaining survivor against all remaining survivors, tiled through LDS the same way; it sets the
//               survivors' mask bytes and leaves one count per workgroup, which count_kernel adds in index order.
// The launches are separate and plain; omb_api.hip reads the survivor counts between them to size the next one.
//
// Filtering against survivors alone is exact: dominance on NaN-free points is a strict partial order, so whatever a
// pass drops is dominated by a point that nothing dominates, and such a point is never dropped.  The mask is therefore
// a function of the set alone: the order in which the survivors land in a list (a slot counter per set, one atomic
// per wavefront — the only atomics here) changes which points share a tile, never the result.
#include "omb_internal.h"

namespace omb {

namespace {

// lane's point p (registers) against ntp tile points (ntp a multiple of 8; the padding is NaN, which dominates
// nobody): false once a tile point dominates p.  The wavefront leaves on a ballot once all its lanes are dead.  U tile
// points per step: as many as keep the 1024-lane workgroup's 128 registers per lane free of spills.
template <int K>
__device__ __forceinline__ bool nd_survives(const double* tile, int ntp, const double (&p)[K], bool alive) {
  constexpr int U = K <= 2 ? 8 : (K <= 4 ? 4 : 2);
  for (int j0 = 0; j0 < ntp; j0 += U) {
    if (__ballot(alive) == 0ull) break;
    bool dom = false;
#pragma unroll
    for (int jj = 0; jj < U; ++jj) {
      const double* q = tile + (size_t)(j0 + jj) * K;
      bool le = true, lt = false;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        const double a = q[c];
        le &= a <= p[c];
        lt |= a < p[c];
      }
      dom |= le & lt;
    }
    alive &= !dom;
  }
  return alive;
}

// Point i of set s into p; true when a coordinate is NaN.
template <int K>
__device__ __forceinline__ bool nd_load(const double* __restrict__ y, int64_t ld, int S, int s, int64_t i,
                                        double (&p)[K]) {
  bool nan = false;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    p[c] = y[((int64_t)c * S + s) * ld + i];
    nan |= p[c] != p[c];
  }
  return nan;
}

template <int K>
__device__ __forceinline__ void nd_stage(double* tile, int t, bool have, const double (&p)[K]) {
#pragma unroll
  for (int c = 0; c < K; ++c) tile[(size_t)t * K + c] = have ? p[c] : __builtin_nan("");
}

// One tile pass.  in == nullptr: the points 0..N-1 themselves (mask bytes cleared, NaN rows dropped); else the
// in_cnt[s] indices of in + s·in_pitch.  Survivors go to out + s·out_pitch at slots taken from out_cnt[s].
template <int K>
__global__ __launch_bounds__(kNdTile) void nd_tile_kernel(const double* __restrict__ y, int64_t ld, int64_t N, int S,
                                                          const int32_t* __restrict__ in, int64_t in_pitch,
                                                          const int32_t* __restrict__ in_cnt,
                                                          int32_t* __restrict__ out, int64_t out_pitch,
                                                          int32_t* __restrict__ out_cnt, uint8_t* __restrict__ mask,
                                                          int64_t ldm) {
  __shared__ double tile[kNdTile * K];
  const int s = blockIdx.y, t = threadIdx.x;
  const int64_t M = in ? (int64_t)in_cnt[s] : N;
  const int64_t t0 = (int64_t)blockIdx.x * kNdTile;
  if (t0 >= M) return;
  const int nt = M - t0 < kNdTile ? (int)(M - t0) : kNdTile;
  const bool have = t < nt;
  int64_t i = 0;
  double p[K] = {};
  bool alive = false;
  if (have) {
    i = in ? (int64_t)in[(int64_t)s * in_pitch + t0 + t] : t0 + t;
    alive = !nd_load<K>(y, ld, S, s, i, p);
    if (!in) mask[(int64_t)s * ldm + i] = 0;
  }
  nd_stage<K>(tile, t, have, p);
  __syncthreads();
  alive = nd_survives<K>(tile, (nt + 7) & ~7, p, alive);
  // compaction: one slot range per wavefront
  const unsigned long long b = __ballot(alive);
  const int lane = t & 63;
  int base = 0;
  if (lane == 0 && b) base = atomicAdd(out_cnt + s, (int)__popcll(b));
  base = __shfl(base, 0);
  if (alive) out[(int64_t)s * out_pitch + base + (int)__popcll(b & ((1ull << lane) - 1ull))] = (int32_t)i;
}

// The final pass over the cnt[s] survivors of list + s·pitch: every one against all of them.  Sets the mask bytes of
// those nothing dominates and leaves this workgroup's number of them in blockcnt[s·gridDim.x + blockIdx.x].
template <int K>
__global__ __launch_bounds__(kNdTile) void nd_final_kernel(const double* __restrict__ y, int64_t ld, int S,
                                                           const int32_t* __restrict__ list, int64_t pitch,
                                                           const int32_t* __restrict__ cnt, uint8_t* __restrict__ mask,
                                                           int64_t ldm, int32_t* __restrict__ blockcnt) {
  __shared__ double tile[kNdTile * K];
  const int s = blockIdx.y, t = threadIdx.x;
  const int64_t M = cnt[s];
  const int64_t t0 = (int64_t)blockIdx.x * kNdTile;
  int32_t* mine = blockcnt + (int64_t)s * gridDim.x + blockIdx.x;
  if (t0 >= M) {
    if (t == 0) *mine = 0;
    return;
  }
  const int32_t* ls = list + (int64_t)s * pitch;
  int64_t i = 0;
  double p[K] = {};
  bool alive = t0 + t < M;
  if (alive) {
    i = ls[t0 + t];
    (void)nd_load<K>(y, ld, S, s, i, p);   // the first pass dropped the NaN rows
  }
  for (int64_t j0 = 0; j0 < M; j0 += kNdTile) {
    const int nt = M - j0 < kNdTile ? (int)(M - j0) : kNdTile;
    double q[K] = {};
    const bool have = t < nt;
    if (have) (void)nd_load<K>(y, ld, S, s, ls[j0 + t], q);
    __syncthreads();   // the previous tile is read
    nd_stage<K>(tile, t, have, q);
    __syncthreads();
    alive = nd_survives<K>(tile, (nt + 7) & ~7, p, alive);
  }
  if (alive) mask[(int64_t)s * ldm + i] = 1;
  // the workgroup's count: one slot per wavefront in the tile's place, added in wavefront order
  const unsigned long long b = __ballot(alive);
  __syncthreads();
  int* w = reinterpret_cast<int*>(tile);
  if ((t & 63) == 0) w[t >> 6] = (int)__popcll(b);
  __syncthreads();
  if (t == 0) {
    int n = 0;
    for (int v = 0; v < kNdTile / 64; ++v) n += w[v];
    *mine = n;
  }
}

// count[s] = Σ_b blockcnt[s·nb + b], lanes striding the row and a tree over the workgroup: integers, in a fixed order.
__global__ __launch_bounds__(256) void nd_count_kernel(const int32_t* __restrict__ blockcnt, int nb,
                                                       int64_t* __restrict__ count) {
  __shared__ long long part[256];
  const int s = blockIdx.x, t = threadIdx.x;
  long long n = 0;
  for (int b = t; b < nb; b += 256) n += blockcnt[(int64_t)s * nb + b];
  part[t] = n;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) part[t] += part[t + h];
    __syncthreads();
  }
  if (t == 0) count[s] = part[0];
}

template <int K>
hipError_t tile_k(hipStream_t stream, int S, const double* y, int64_t ld, int64_t N, const int32_t* in,
                  int64_t in_pitch, const int32_t* in_cnt, int64_t Mmax, int32_t* out, int64_t out_pitch,
                  int32_t* out_cnt, uint8_t* mask, int64_t ldm) {
  const unsigned nb = (unsigned)((Mmax + kNdTile - 1) / kNdTile);
  hipLaunchKernelGGL(nd_tile_kernel<K>, dim3(nb, S), dim3(kNdTile), 0, stream, y, ld, N, S, in, in_pitch, in_cnt, out,
                     out_pitch, out_cnt, mask, ldm);
  return hipGetLastError();
}

template <int K>
hipError_t final_k(hipStream_t stream, int S, const double* y, int64_t ld, const int32_t* list, int64_t pitch,
                   const int32_t* cnt, unsigned nb, uint8_t* mask, int64_t ldm, int32_t* blockcnt) {
  hipLaunchKernelGGL(nd_final_kernel<K>, dim3(nb, S), dim3(kNdTile), 0, stream, y, ld, S, list, pitch, cnt, mask, ldm,
                     blockcnt);
  return hipGetLastError();
}

}  // namespace

#define OMB_ND_DISPATCH(fn, ...)            \
  switch (k) {                              \
    case 1: return fn<1>(__VA_ARGS__);      \
    case 2: return fn<2>(__VA_ARGS__);      \
    case 3: return fn<3>(__VA_ARGS__);      \
    case 4: return fn<4>(__VA_ARGS__);      \
    case 5: return fn<5>(__VA_ARGS__);      \
    case 6: return fn<6>(__VA_ARGS__);      \
    case 7: return fn<7>(__VA_ARGS__);      \
    case 8: return fn<8>(__VA_ARGS__);      \
    default: return hipErrorInvalidValue;   \
  }

hipError_t launch_nd_tile(hipStream_t stream, int k, int S, const double* y, int64_t ld, int64_t N, const int32_t* in,
                          int64_t in_pitch, const int32_t* in_cnt, int64_t Mmax, int32_t* out, int64_t out_pitch,
                          int32_t* out_cnt, uint8_t* mask, int64_t ldm) {
  if (S < 1 || S > kNdMaxS || Mmax < 1 || Mmax > kNdMaxN || (in ? Mmax > in_pitch : Mmax != N) || out_pitch < Mmax)
    return hipErrorInvalidValue;
  OMB_ND_DISPATCH(tile_k, stream, S, y, ld, N, in, in_pitch, in_cnt, Mmax, out, out_pitch, out_cnt, mask, ldm)
}

hipError_t launch_nd_final(hipStream_t stream, int k, int S, const double* y, int64_t ld, const int32_t* list,
                           int64_t pitch, const int32_t* cnt, int64_t Mmax, uint8_t* mask, int64_t ldm,
                           int32_t* blockcnt, int64_t* count) {
  if (S < 1 || S > kNdMaxS || Mmax < 0 || Mmax > kNdMaxN || Mmax > pitch) return hipErrorInvalidValue;
  const unsigned nb = (unsigned)nd_final_blocks(Mmax);
  hipError_t e = hipSuccess;
  {
    auto go = [&]() -> hipError_t {
      OMB_ND_DISPATCH(final_k, stream, S, y, ld, list, pitch, cnt, nb, mask, ldm, blockcnt)
    };
    e = go();
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nd_count_kernel, dim3(S), dim3(256), 0, stream, blockcnt, (int)nb, count);
  return hipGetLastError();
}

}  // namespace omb
