// Exact hypervolume and per-point contributions on gfx950: omb_hypervolume, omb_hypervolume_contrib.
//
// Minimisation, reference point r, point sets in omb_nondominated's layout: coordinate j of point i of set s is
// y[(j·S + s)·ld + i], the row is in the set when mask[s·ldm + i] != 0 (a null mask: every row).  A row is kept when
// every coordinate is finite and < r_j; at most kHvPoints rows of a set may be kept.
//
// A grid sweep.  Objectives 0..k-3 are grid objectives: the sorted distinct values u_j[0..n_j) of the kept points,
// followed by r_j, cut objective j into n_j intervals.  A cell c = (c_0..c_{k-3}) has weight
// w(c) = Π_j (u_j[c_j + 1] − u_j[c_j]), multiplied left to right, and inside it the dominated region is a prism over
// the two-dimensional staircase of the points with rank_j(p) ≤ c_j for every grid objective — exactly the points that
// dominate some (hence every) point of the cell's interior in the grid objectives.  With the points sorted once by
// (y_{k-2}, y_{k-1}) the staircase's area A(c) is one walk: ymin = r_{k-1}; a qualifying point with y_{k-1} < ymin
// adds (r_{k-2} − y_{k-2})·(ymin − y_{k-1}) and becomes ymin.  HV = Σ_c w(c)·A(c).  The cells tile the box below r,
// so the formula is right for any point set: dominated points, duplicates and ties need no special case.  k = 2 is
// one cell of weight 1; k = 1 is the same walk over (0, y_0) against (1, r_0): its first point adds 1·(r_0 − min).
//
//   hv_prep_kernel<K>    one workgroup of kHvPoints lanes per set: filters and compacts the rows in index order
//                        (ballot prefix, no atomics), sorts the kept ones by (y_{k-2}, y_{k-1}, index) with a bitonic
//                        sort in LDS, ranks every grid objective by all-pairs counts, and leaves the sorted pairs, the
//                        packed 16-bit ranks, the grids and n, n_0..n_{k-3} in the context's workspace (HvSet, header).
//   hv_cells_kernel<K>   kHvCellLanes lanes × kHvCellsPerLane cells each; the set's points live in LDS (28 KiB, and 4 KiB for the sum) and
//                        every lane reads the same point per step (a broadcast); only the update is predicated.  The
//                        rank test of a cell is two integer operations: the ranks are 16-bit fields, and
//                        ((c | 0x8000) − rank) keeps bit 15 of a field exactly when c ≥ rank (no borrow crosses a
//                        field, ranks and c being < 2^15).  blockIdx.y is the set, or, for contributions, the variant:
//                        0 the whole set, v + 1 the set without sorted point v — over the same grid, which stays a
//                        valid grid for every subset.
//   hv_reduce_kernel     512 partial sums → 1, a tree of fixed shape; the host repeats it until one value is left.
// The additions form a tree over the cell index alone: a lane adds its kHvCellsPerLane cells in order, a workgroup
// its lanes by halving, hv_reduce_kernel 512 consecutive partials by pairing neighbours and halving.  Workgroups and
// lanes past a set's cells add +0.0, which changes no bit, so the value does not depend on the launch shape, on the
// other sets of the call or on the set's slot.  Plain launches; omb_api.hip reads n and n_j between prep and cells.
#include "omb_internal.h"

#pragma clang fp contract(off)   // a·b + c as written: the numpy restatement's roundings (tests/_hypervolume_reference.py)

namespace omb {

namespace {

constexpr uint64_t kHvHi64 = 0x8000800080008000ull;
constexpr uint32_t kHvHi32 = 0x80008000u;

template <int K>
__global__ __launch_bounds__(kHvPoints) void hv_prep_kernel(const double* __restrict__ y, int64_t ld, int64_t N, int S,
                                                            const uint8_t* __restrict__ mask, int64_t ldm, HvRef ref,
                                                            int32_t* __restrict__ hdr, HvSet* __restrict__ sets) {
  constexpr int G = K > 2 ? K - 2 : 0;
  constexpr int U = 4;                      // sub-chunks of kHvPoints rows per barrier of the compaction
  constexpr int W = kHvPoints / 64;         // wavefronts
  __shared__ int32_t idx[kHvPoints];        // kept rows in index order; later slot → sorted position
  __shared__ int32_t wcnt[2][U][W];
  __shared__ double ka[kHvPoints], kb[kHvPoints];
  __shared__ int32_t ki[kHvPoints];
  __shared__ double val[kHvPoints], fval[kHvPoints];
  const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint8_t* ms = mask ? mask + (int64_t)s * ldm : nullptr;

  // ---- filter and compact: slot = rows kept before this one
  int base = 0;
  int par = 0;
  for (int64_t i0 = 0; i0 < N && base <= kHvPoints; i0 += (int64_t)U * kHvPoints, par ^= 1) {
    unsigned long long b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + (int64_t)u * kHvPoints + t;
      bool keep = i < N && (!ms || ms[i] != 0);
      if (keep) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
          const double v = y[((int64_t)c * S + s) * ld + i];
          keep &= v < ref.r[c] && v > -__builtin_inf();   // NaN, ±inf and v ≥ r_c drop the row
        }
      }
      b[u] = __ballot(keep);
      if (lane == 0) wcnt[par][u][wave] = (int)__popcll(b[u]);
    }
    __syncthreads();   // wcnt[par] is complete; wcnt[par ^ 1] is next written after the following barrier
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const int cw = wcnt[par][u][w];
        before += w < wave ? cw : 0;
        total += cw;
      }
      if ((b[u] >> lane) & 1ull) {
        const int slot = base + before + (int)__popcll(b[u] & ((1ull << lane) - 1ull));
        if (slot < kHvPoints) idx[slot] = (int32_t)(i0 + (int64_t)u * kHvPoints + t);
      }
      base += total;
    }
  }
  __syncthreads();
  const int n = base;
  if (t == 0) hdr[s * kHvHdr] = n;          // above kHvPoints: "more than", the scan stopped there
  if (n > kHvPoints || n == 0) {
    if (t < G) hdr[s * kHvHdr + 1 + t] = 0;
    return;
  }
  HvSet* out = sets + s;

  // ---- the kept points: lane t holds slot t
  const bool have = t < n;
  const int32_t row = have ? idx[t] : 0;
  double p[K];
#pragma unroll
  for (int c = 0; c < K; ++c) p[c] = have ? y[((int64_t)c * S + s) * ld + row] : 0.0;
  const double px = K >= 2 ? p[K >= 2 ? K - 2 : 0] : 0.0, py = p[K - 1];

  // ---- bitonic sort of (x, y, slot); the padding sorts last
  ka[t] = have ? px : __builtin_inf();
  kb[t] = have ? py : __builtin_inf();
  ki[t] = t;
  __syncthreads();
  for (int size = 2; size <= kHvPoints; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int q = t ^ stride;
      if (q > t) {
        const double a0 = ka[t], b0 = kb[t], a1 = ka[q], b1 = kb[q];
        const int i0 = ki[t], i1 = ki[q];
        const bool gt = a0 > a1 || (a0 == a1 && (b0 > b1 || (b0 == b1 && i0 > i1)));
        if (gt == ((t & size) == 0)) {
          ka[t] = a1, kb[t] = b1, ki[t] = i1;
          ka[q] = a0, kb[q] = b0, ki[q] = i0;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();                          // idx's rows are in registers: it now maps slot → sorted position
  if (have) idx[ki[t]] = t;
  __syncthreads();
  const int pos = have ? idx[t] : 0;
  if (have) {
    out->xs[pos] = px;
    out->ys[pos] = py;
    out->orig[pos] = row;
  }

  // ---- ranks and grids of the grid objectives: all-pairs counts over the first occurrence of every value
  uint64_t rlo = 0;
  uint32_t rhi = 0;
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const double v = p[j];
    __syncthreads();                        // the previous objective's fval is read
    val[t] = have ? v : __builtin_nan("");
    __syncthreads();
    bool first = have;
    for (int u = 0; u < n; ++u) first &= !(u < t && val[u] == v);
    fval[t] = first ? v : __builtin_nan("");
    __syncthreads();
    int rank = 0, nj = 0;
    for (int u = 0; u < n; ++u) {
      const double f = fval[u];
      rank += f < v ? 1 : 0;
      nj += f == f ? 1 : 0;
    }
    if (first) out->grid[j][rank] = v;
    if (t == 0) {
      out->grid[j][nj] = ref.r[j];
      hdr[s * kHvHdr + 1 + j] = nj;
    }
    if (j < 4) rlo |= (uint64_t)rank << (16 * j);
    else rhi |= (uint32_t)rank << (16 * (j - 4));
  }
  if (have) {
    out->rlo[pos] = rlo;
    out->rhi[pos] = rhi;
  }
}

template <int K>
__global__ __launch_bounds__(kHvCellLanes) void hv_cells_kernel(const int32_t* __restrict__ hdr,
                                                                const HvSet* __restrict__ sets, HvRef ref,
                                                                int per_point, double* __restrict__ partials,
                                                                int64_t pitch) {
  constexpr int G = K > 2 ? K - 2 : 0;
  constexpr int C = kHvCellsPerLane;
  __shared__ double2 xy[kHvPoints];
  __shared__ uint64_t rlo[kHvPoints];
  __shared__ uint32_t rhi[kHvPoints];
  __shared__ double part[kHvCellLanes];
  const int t = threadIdx.x;
  const int s = per_point ? 0 : (int)blockIdx.y;
  const int skip = per_point ? (int)blockIdx.y - 1 : -1;
  double* mine = partials + (int64_t)blockIdx.y * pitch + blockIdx.x;
  const int n = hdr[s * kHvHdr];
  int nj[G > 0 ? G : 1];
  int64_t cells = (n >= 1 && n <= kHvPoints) ? 1 : 0;
#pragma unroll
  for (int j = 0; j < G; ++j) {
    nj[j] = hdr[s * kHvHdr + 1 + j];
    cells *= nj[j];
  }
  const int64_t base = (int64_t)blockIdx.x * kHvBlockCells;
  if (base >= cells) {                      // past this set's cells (or an empty set): +0.0, which changes no sum
    if (t == 0) *mine = 0.0;
    return;
  }
  const HvSet* in = sets + s;
  for (int i = t; i < n; i += kHvCellLanes) {
    xy[i] = make_double2(in->xs[i], in->ys[i]);
    rlo[i] = in->rlo[i];
    rhi[i] = in->rhi[i];
  }
  const double rx = K >= 2 ? ref.r[K >= 2 ? K - 2 : 0] : 1.0, ry = ref.r[K - 1];

  // ---- this lane's cells: base + e·kHvCellLanes + t, their ranks packed like the points' and their weights
  // (the first is split by mixed radix, objective 0 the slowest digit; the others step it by kHvCellLanes with carries)
  uint64_t clo[C];
  uint32_t chi[C];
  double w[C], ymin[C], A[C];
  unsigned dig[G > 0 ? G : 1] = {};
  {
    int64_t rem = base + t < cells ? base + t : 0;
#pragma unroll
    for (int j = G - 1; j >= 0; --j) {
      dig[j] = (unsigned)(rem % nj[j]);
      rem /= nj[j];
    }
  }
#pragma unroll
  for (int e = 0; e < C; ++e) {
    const bool valid = base + (int64_t)e * kHvCellLanes + t < cells;
    if (e > 0) {
      unsigned carry = kHvCellLanes;
#pragma unroll
      for (int j = G - 1; j >= 0; --j) {
        const unsigned v = dig[j] + carry, m = (unsigned)nj[j];
        carry = v / m;
        dig[j] = v - carry * m;
      }
    }
    int cj[G > 0 ? G : 1] = {};
#pragma unroll
    for (int j = 0; j < G; ++j) cj[j] = valid ? (int)dig[j] : 0;   // past the last cell the carry leaves the grid
    uint64_t lo = 0;
    uint32_t hi = 0;
    double we = 1.0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const double d = in->grid[j][cj[j] + 1] - in->grid[j][cj[j]];
      we = j == 0 ? d : we * d;
      if (j < 4) lo |= (uint64_t)cj[j] << (16 * j);
      else hi |= (uint32_t)cj[j] << (16 * (j - 4));
    }
    clo[e] = lo | kHvHi64;
    chi[e] = hi | kHvHi32;
    w[e] = valid ? we : 0.0;
    ymin[e] = ry;
    A[e] = 0.0;
  }
  __syncthreads();

  // ---- the walk: one LDS broadcast per point, C predicated updates
  for (int i = 0; i < n; ++i) {
    if (i == skip) continue;
    const double2 q = xy[i];
    const uint64_t pl = rlo[i];
    const uint32_t ph = rhi[i];
    const double dx = rx - q.x;
#pragma unroll
    for (int e = 0; e < C; ++e) {
      bool ok = ((clo[e] - pl) & kHvHi64) == kHvHi64;
      if (G > 4) ok &= ((chi[e] - ph) & kHvHi32) == kHvHi32;
      if (ok && q.y < ymin[e]) {
        A[e] += dx * (ymin[e] - q.y);
        ymin[e] = q.y;
      }
    }
  }

  // ---- Σ w·A: the lane's cells in order, then the workgroup by halving
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < C; ++e) acc += w[e] * A[e];
  part[t] = acc;
  __syncthreads();
  for (int h = kHvCellLanes / 2; h > 0; h >>= 1) {
    if (t < h) part[t] += part[t + h];
    __syncthreads();
  }
  if (t == 0) *mine = part[0];
}

// out[v·out_pitch + b] = the sum of in[v·in_pitch + 512·b .. + 512) (zeros past nb): neighbours paired, then halving.
__global__ __launch_bounds__(kHvReduceLanes) void hv_reduce_kernel(const double* __restrict__ in, int64_t nb,
                                                                   int64_t in_pitch, double* __restrict__ out,
                                                                   int64_t out_pitch) {
  __shared__ double part[kHvReduceLanes];
  const int t = threadIdx.x;
  const double* row = in + (int64_t)blockIdx.y * in_pitch;
  const int64_t i = ((int64_t)blockIdx.x * kHvReduceLanes + t) * 2;
  const double a = i < nb ? row[i] : 0.0, b = i + 1 < nb ? row[i + 1] : 0.0;
  part[t] = a + b;
  __syncthreads();
  for (int h = kHvReduceLanes / 2; h > 0; h >>= 1) {
    if (t < h) part[t] += part[t + h];
    __syncthreads();
  }
  if (t == 0) out[(int64_t)blockIdx.y * out_pitch + blockIdx.x] = part[0];
}

// tot[0] = HV(set), tot[v + 1] = HV(set without sorted point v): hv and the kept rows' contributions.
__global__ __launch_bounds__(kHvPoints) void hv_contrib_kernel(const double* __restrict__ tot,
                                                               const int32_t* __restrict__ hdr,
                                                               const HvSet* __restrict__ set, double* __restrict__ hv,
                                                               double* __restrict__ contrib) {
  const int t = threadIdx.x, n = hdr[0];
  if (t == 0) *hv = tot[0];
  if (t < n && n <= kHvPoints) contrib[set->orig[t]] = tot[0] - tot[t + 1];
}

template <int K>
hipError_t prep_k(hipStream_t stream, int S, const double* y, int64_t ld, int64_t N, const uint8_t* mask, int64_t ldm,
                  const HvRef& ref, int32_t* hdr, HvSet* sets) {
  hipLaunchKernelGGL(hv_prep_kernel<K>, dim3(S), dim3(kHvPoints), 0, stream, y, ld, N, S, mask, ldm, ref, hdr, sets);
  return hipGetLastError();
}

template <int K>
hipError_t cells_k(hipStream_t stream, unsigned nb, int V, int per_point, const int32_t* hdr, const HvSet* sets,
                   const HvRef& ref, double* partials) {
  hipLaunchKernelGGL(hv_cells_kernel<K>, dim3(nb, V), dim3(kHvCellLanes), 0, stream, hdr, sets, ref, per_point,
                     partials, (int64_t)nb);
  return hipGetLastError();
}

}  // namespace

#define OMB_HV_DISPATCH(fn, ...)            \
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

hipError_t launch_hv_prep(hipStream_t stream, int k, int S, const double* y, int64_t ld, int64_t N,
                          const uint8_t* mask, int64_t ldm, const HvRef& ref, int32_t* hdr, HvSet* sets) {
  if (S < 1 || S > kHvMaxS || N < 1 || N > kHvMaxN || ld < N || (mask && ldm < N)) return hipErrorInvalidValue;
  OMB_HV_DISPATCH(prep_k, stream, S, y, ld, N, mask, ldm, ref, hdr, sets)
}

hipError_t launch_hv_cells(hipStream_t stream, int k, int V, bool per_point, int64_t max_cells, const int32_t* hdr,
                           const HvSet* sets, const HvRef& ref, double* partials, double* scratch, double* out) {
  const int64_t nb = hv_cell_blocks(max_cells);
  // a launch counts its lanes per dimension in 32 bits (the work cap keeps a call three times below that)
  if (V < 1 || V > kHvPoints + 1 || (!per_point && V > kHvMaxS) || max_cells < 0 ||
      nb > (int64_t)(UINT32_MAX / kHvCellLanes))
    return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  {
    auto go = [&]() -> hipError_t {
      OMB_HV_DISPATCH(cells_k, stream, (unsigned)nb, V, per_point ? 1 : 0, hdr, sets, ref, partials)
    };
    e = go();
  }
  if (e != hipSuccess) return e;
  // partials (V, nb) → scratch (V, ⌈nb/512⌉) → partials … until one value per row is left, which goes to out[v]
  const double* in = partials;
  double* other = scratch;
  int64_t m = nb;
  for (;;) {
    const int64_t mo = hv_reduce_blocks(m);
    double* dst = mo == 1 ? out : other;
    hipLaunchKernelGGL(hv_reduce_kernel, dim3((unsigned)mo, V), dim3(kHvReduceLanes), 0, stream, in, m, m, dst, mo);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (mo == 1) return hipSuccess;
    other = const_cast<double*>(in);
    in = dst;
    m = mo;
  }
}

hipError_t launch_hv_contrib(hipStream_t stream, const double* tot, const int32_t* hdr, const HvSet* set, double* hv,
                             double* contrib) {
  hipLaunchKernelGGL(hv_contrib_kernel, dim3(1), dim3(kHvPoints), 0, stream, tot, hdr, set, hv, contrib);
  return hipGetLastError();
}

}  // namespace omb
