// cluster_kernels.hip -- the fine stage's per-coarse-patch clustering (MicArray._cluster_group,
// sep/Mic_Array.py:283-383) for all coarse patches of a call, as fine_cluster.fine_clusters_f64 states it: float64, no
// logarithm, one fixed order of additions -- every value below is the statement's value to the bit.  The second half of
// the file is the global clustering's walk (MicArray.Clustering_new) as global_cluster.global_clusters_f64 states it, and the
// last part the coarse stage's decision over a lattice as search.coarse_select_f64 states it.
#include "asw_common.h"

#include <vector>

namespace {

constexpr int GR = 8;                            // a workgroup of group_gram_kernel owns GR x GR row pairs
constexpr long GRAM_MAX_ELEMS = 1L << 27;        // cap of sum n_g^2 per call (1 GiB of float64)

// ---------------------------------------------------------------------------
// group_gram_kernel: G[a][b] = sum_t double(y_a[t]) * double(y_b[t]) for the row pairs of every group, one launch.
// Workgroup w reads (group, tile row ta, tile column tb >= ta) from tiles[2w], tiles[2w + 1] = ta << 16 | tb.  Thread l
// sums t = l, l + 256, ... from 0.0 with 4-byte loads -- coalesced whatever the alignment of a row --, a float32 x
// float32 product being exact in double so that the fused multiply-add rounds the statement's sum.  Then the
// statement's reduction: the butterfly p[l] += p[l + s], s = 32 .. 1, inside each wavefront (one 64-wide quarter), and
// (w0 + w1) + (w2 + w3) over the four through LDS.  A row past the ragged edge of the group repeats the group's last
// row and its pairs are not stored, so the kept pairs do not see the edge.  Both halves of an off-diagonal tile are
// stored from the one sum; inside a diagonal tile [i][j] and [j][i] add the same products in the same order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_gram_kernel(const float* __restrict__ y, int T, const int* __restrict__ bounds,
                                                         const int* __restrict__ goff, const int* __restrict__ tiles,
                                                         double* __restrict__ gram) {
  __shared__ double red[4][GR * GR];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = tiles[2 * blockIdx.x], tt = tiles[2 * blockIdx.x + 1];
  const int ta = tt >> 16, tb = tt & 0xffff;
  const int b0 = bounds[g], n = bounds[g + 1] - b0;
  const float* ra[GR];
  const float* rb[GR];
#pragma unroll
  for (int i = 0; i < GR; ++i) {
    const int a = ta * GR + i, b = tb * GR + i;
    ra[i] = y + (long)(b0 + (a < n ? a : n - 1)) * T;
    rb[i] = y + (long)(b0 + (b < n ? b : n - 1)) * T;
  }
  double acc[GR][GR];
#pragma unroll
  for (int i = 0; i < GR; ++i)
#pragma unroll
    for (int j = 0; j < GR; ++j) acc[i][j] = 0.0;
  for (int t = tid; t < T; t += 256) {
    double va[GR], vb[GR];
#pragma unroll
    for (int i = 0; i < GR; ++i) {
      va[i] = (double)ra[i][t];
      vb[i] = (double)rb[i][t];
    }
#pragma unroll
    for (int i = 0; i < GR; ++i)
#pragma unroll
      for (int j = 0; j < GR; ++j) acc[i][j] = __builtin_fma(va[i], vb[j], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < GR; ++i)
#pragma unroll
    for (int j = 0; j < GR; ++j) {
      double p = acc[i][j];
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) p = p + __shfl_down(p, s, 64);     // lanes < s hold the statement's p[:s]
      if (lane == 0) red[wid][i * GR + j] = p;
    }
  __syncthreads();
  if (tid < GR * GR) {
    const double v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    const int a = ta * GR + tid / GR, b = tb * GR + tid % GR;
    if (a < n && b < n) {
      double* __restrict__ out = gram + goff[g];
      out[(long)a * n + b] = v;
      if (ta != tb) out[(long)b * n + a] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// fine_cluster_kernel: one wavefront per group.  (1) order[] of the group := its rows in index order, so that every
// slot holds a row of the group whatever the powers are; the open flag: max power2 >= group_gate.  (2) each candidate's
// place in the visiting order by counting the candidates that go before it -- larger power, or equal power and a lower
// index -- O(n^2), any n.  (3) the greedy loop over the visiting order, serial in the candidates: the lanes test the
// current one against 64 heads at a time, the ballot's lowest set bit is the first head in creation order; a group
// with more heads takes more rounds.  The head list is `heads` (workspace, the group's own n slots): nothing is sized
// by LDS.  The wavefront is the whole workgroup, so __syncthreads() here is the fence that lets every lane read what
// another lane stored to global memory.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void fine_cluster_kernel(const double* __restrict__ energies, const double* __restrict__ gate,
                                                          const double* __restrict__ group_gate, double min_trigger, double ratio,
                                                          const int* __restrict__ bounds, const int* __restrict__ goff,
                                                          const double* __restrict__ gram, int* __restrict__ heads,
                                                          int* __restrict__ order, int* __restrict__ label) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const int b0 = bounds[g], n = bounds[g + 1] - b0;
  if (n <= 0) return;                                               // the whole workgroup leaves
  const double* __restrict__ en = energies + (long)b0 * 2;
  double top = -__builtin_inf();
  for (int i = lane; i < n; i += 64) {
    order[b0 + i] = b0 + i;
    label[b0 + i] = -1;
    const double v = en[2 * i + 1];
    top = v > top ? v : top;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(top, o, 64);
    top = w > top ? w : top;
  }
  const bool open = !(top < group_gate[g]);
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const double p = en[2 * i];
    int before = 0;
    for (int j = 0; j < n; ++j) {
      const double q = en[2 * j];
      before += (q > p || (q == p && j < i)) ? 1 : 0;
    }
    if (before < n) order[b0 + before] = b0 + i;                    // always true; spelled out for the reader of bounds
  }
  __syncthreads();
  if (!open) return;
  const double* __restrict__ G = gram + goff[g];
  int* __restrict__ hd = heads + b0;
  int nh = 0;
  for (int r = 0; r < n; ++r) {
    int k = order[b0 + r] - b0;
    k = k < 0 ? 0 : (k >= n ? n - 1 : k);                           // (a row of the group by construction)
    if (en[2 * k + 1] < gate[b0 + k] || en[2 * k] < min_trigger) continue;    // wave-uniform
    const double ee = G[(long)k * n + k];
    int home = -1;
    for (int c = 0; c < nh && home < 0; c += 64) {
      const int h = c + lane < nh ? hd[c + lane] : -1;
      bool same = false;
      if (h >= 0) {
        const double ss = G[(long)h * n + h], es = G[(long)k * n + h];
        const double sss = es * es / ss;
        double snn = ee - sss;
        snn = (snn > 0.0 ? snn : 0.0) + 1e-8;
        same = sss > ratio * snn;
      }
      const unsigned long long hit = __ballot(same);
      if (hit) home = __shfl(h, __builtin_ctzll(hit), 64);
    }
    if (home < 0) {
      if (lane == 0) {
        hd[nh] = k;
        label[b0 + k] = b0 + k;
      }
      ++nh;
      __syncthreads();                                              // the next candidate's lanes read hd[]
    } else if (lane == 0) {
      label[b0 + k] = b0 + home;
    }
  }
}

// bounds[G + 1] checked: starts at 0, does not decrease, ends at N; -> sum n_g^2 and the number of tiles
int check_bounds(const char* who, const int32_t* bounds, int G, long N, long* elems, long* n_tiles) {
  ASW_CHECK_ARG(G >= 0 && G <= 65535, "%s: G = %d outside 0..65535", who, G);
  ASW_CHECK_ARG(bounds, "%s: null bounds", who);
  ASW_CHECK_ARG(bounds[0] == 0, "%s: bounds[0] = %d, not 0", who, bounds[0]);
  long e = 0, nt = 0;
  for (int g = 0; g < G; ++g) {
    const long n = (long)bounds[g + 1] - bounds[g];
    ASW_CHECK_ARG(n >= 0, "%s: bounds decrease at group %d (%d after %d)", who, g, bounds[g + 1], bounds[g]);
    e += n * n;
    ASW_CHECK_ARG(e <= GRAM_MAX_ELEMS, "%s: sum of n_g^2 exceeds the cap of %ld elements at group %d", who, GRAM_MAX_ELEMS, g);
    const long t = (n + GR - 1) / GR;
    nt += t * (t + 1) / 2;
  }
  ASW_CHECK_ARG(N < 0 || bounds[G] == N, "%s: bounds[G] = %d, not N = %ld", who, bounds[G], N);
  *elems = e;
  *n_tiles = nt;
  return ASW_OK;
}

// workspace: [elems] float64 Gram | int32: bounds [G + 1] | goff [G + 1] | tiles [2 n_tiles] | heads [N]
size_t workspace_need(long elems, int G, long n_tiles, long N) {
  return (size_t)elems * sizeof(double) + ((size_t)2 * (G + 1) + (size_t)2 * n_tiles + (size_t)N) * sizeof(int32_t);
}

}  // namespace

extern "C" size_t asw_fine_clusters_workspace_bytes(const int32_t* bounds_host, int G) {
  long elems = 0, n_tiles = 0;
  if (check_bounds("fine_clusters_workspace_bytes", bounds_host, G, -1, &elems, &n_tiles) != ASW_OK) return 0;
  return workspace_need(elems, G, n_tiles, bounds_host[G]);
}

extern "C" int asw_fine_clusters(const float* y, int N, int T, const int32_t* bounds_host, int G, const double* energies,
                                 const double* gate, const double* group_gate, double min_trigger, double ratio,
                                 void* workspace, size_t workspace_bytes, int32_t* order, int32_t* label, double* gram,
                                 void* stream) {
  ASW_CHECK_ARG(N >= 0, "fine_clusters: N = %d < 0", N);
  ASW_CHECK_ARG(T >= 1, "fine_clusters: T = %d < 1", T);
  long elems = 0, n_tiles = 0;
  if (int rc = check_bounds("fine_clusters", bounds_host, G, N, &elems, &n_tiles)) return rc;
  if (N == 0 || G == 0) return ASW_OK;
  ASW_CHECK_ARG(y && energies && gate && group_gate && workspace, "fine_clusters: null pointer");
  ASW_CHECK_ARG(order && label, "fine_clusters: null output");
  const size_t need = workspace_need(elems, G, n_tiles, N);
  ASW_CHECK_ARG(workspace_bytes >= need, "fine_clusters: workspace of %zu bytes too small, %zu needed", workspace_bytes, need);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "fine_clusters: workspace not 8-byte aligned");

  // the small table both kernels read: group bounds, Gram offsets, workgroup -> (group, tile)
  std::vector<int32_t> table((size_t)2 * (G + 1) + (size_t)2 * n_tiles);
  int32_t* hb = table.data();
  int32_t* ho = hb + (G + 1);
  int32_t* ht = ho + (G + 1);
  long e = 0, w = 0;
  for (int g = 0; g <= G; ++g) {
    hb[g] = bounds_host[g];
    ho[g] = (int32_t)e;
    if (g == G) break;
    const long n = (long)bounds_host[g + 1] - bounds_host[g], t = (n + GR - 1) / GR;
    for (long a = 0; a < t; ++a)
      for (long b = a; b < t; ++b) {
        ht[2 * w] = g;
        ht[2 * w + 1] = (int32_t)(a << 16 | b);                     // t <= 1449 under the cap
        ++w;
      }
    e += n * n;
  }
  hipStream_t s = asw::as_stream(stream);
  double* gram_ws = static_cast<double*>(workspace);
  int32_t* db = reinterpret_cast<int32_t*>(gram_ws + elems);
  int32_t* dofs = db + (G + 1);
  int32_t* dt = dofs + (G + 1);
  int32_t* heads = dt + 2 * n_tiles;
  double* gm = gram ? gram : gram_ws;
  // pageable source: the runtime has taken the table before the call returns
  ASW_HIP(hipMemcpyAsync(db, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  {
    asw::ProfScope prof(s, "group_gram", 2.0 * (double)elems * T, 0.0);
    hipLaunchKernelGGL(group_gram_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, y, T, db, dofs, dt, gm);
    ASW_LAUNCH_CHECK();
  }
  asw::ProfScope prof(s, "fine_cluster", 0.0, (double)elems * 8);
  hipLaunchKernelGGL(fine_cluster_kernel, dim3(G), dim3(64), 0, s, energies, gate, group_gate, min_trigger, ratio, db, dofs,
                     gm, heads, order, label);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

// ===========================================================================
// The global clustering (MicArray.Clustering_new, sep/Mic_Array.py:399-500) as global_cluster.global_clusters_f64 states
// it: comparisons of the float64 values pair_sisdr and segment_sisdr wrote, a first-hit scan and a running maximum.
// There is no arithmetic, so every decision below is the statement's on every input, NaN and Inf included (a NaN
// compares false on both sides of every test, as in numpy).
// ===========================================================================
namespace {

constexpr int GLOBAL_MAX_ROWS = 8192;            // n * n bytes of merge matrix: 64 MiB at the cap

__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------
// global_merge_kernel: one wavefront per ordered pair (i, j), four pairs per workgroup.  The lanes stride over the
// used slots k < c_i of seg[i][j][.] -- contiguous doubles, so a wavefront's load is coalesced --, the two "any" flags
// meet by ballot, and lane 0 stores merge[i][j] = full > sim_db or (any > win_hi and no < win_lo) or near.  Slots from
// c_i on are never read.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void global_merge_kernel(const double* __restrict__ full, const double* __restrict__ seg,
                                                           const int* __restrict__ counts, const unsigned char* __restrict__ near,
                                                           int n, int K, double sim_db, double win_hi, double win_lo,
                                                           unsigned char* __restrict__ merge) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long pair = (long)blockIdx.x * 4 + wid;
  if (pair >= (long)n * n) return;                                  // a whole wavefront leaves; no barrier follows
  const int i = (int)(pair / n);
  const int c = clamp_int(counts[i], 0, K);
  const double* __restrict__ row = seg + pair * K;
  bool hi = false, lo = false;
  for (int k = lane; k < c; k += 64) {
    const double v = row[k];
    hi = hi || v > win_hi;
    lo = lo || v < win_lo;
  }
  const bool any_hi = __ballot(hi) != 0ull, any_lo = __ballot(lo) != 0ull;
  if (lane == 0) merge[pair] = (full[pair] > sim_db || (any_hi && !any_lo) || near[pair] != 0) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// global_walk_kernel: one workgroup of 256 threads walks the candidates in order.  The head list is `heads` (workspace,
// one int per candidate), so nothing is sized by LDS and any n and K run.  Per candidate i with c_i > 0:
//   A. the threads stride over the head positions and keep the lowest p with merge[i][heads[p]] set; a wavefront
//      minimum by shuffles, then the minimum of the four through LDS: the first head in creation order.
//   B. no hit and at least one head: the threads stride over k < c_i; each loops over ALL heads and keeps the maximum of
//      seg[i][h][k] that propagates NaN (consecutive lanes read consecutive doubles).  The two flags of the second
//      window test meet by ballot and through LDS.
// Every branch on c_i, the hit and the flags is uniform over the workgroup, so every thread meets the same barriers.
// Thread 0 stores label[i] and the new head; the barrier that ends the step is the fence that lets the other threads
// read heads[] and lets the LDS words be reused.  Every head index read back from memory is clamped to 0 .. n - 1.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void global_walk_kernel(const double* __restrict__ seg, const int* __restrict__ counts,
                                                          const unsigned char* __restrict__ merge, int n, int K,
                                                          double best_hi, double best_lo, int* __restrict__ heads,
                                                          int* __restrict__ label) {
  __shared__ int first[4];
  __shared__ int flag[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int nh = 0;
  for (int i = 0; i < n; ++i) {
    const int c = clamp_int(counts[i], 0, K);
    if (c == 0) {
      if (tid == 0) label[i] = -1;
      continue;
    }
    const unsigned char* __restrict__ mrow = merge + (long)i * n;
    int pos = nh;                                                   // nh = "no hit"
    for (int p = tid; p < nh; p += 256) {
      const int h = clamp_int(heads[p], 0, n - 1);
      if (mrow[h] != 0) {
        pos = p;
        break;                                                      // this thread's later positions are larger
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int w = __shfl_xor(pos, o, 64);
      pos = w < pos ? w : pos;
    }
    if (lane == 0) first[wid] = pos;
    __syncthreads();
    {
      const int a = first[0] < first[1] ? first[0] : first[1], b = first[2] < first[3] ? first[2] : first[3];
      pos = a < b ? a : b;
    }
    if (pos < nh) {
      if (tid == 0) label[i] = clamp_int(heads[pos], 0, n - 1);
      __syncthreads();                                              // first[] is free again
      continue;
    }
    bool shadowed = false;
    if (nh > 0) {
      bool hi = false, lo = false;
      const double* __restrict__ srow = seg + (long)i * n * K;
      for (int k = tid; k < c; k += 256) {
        double best = srow[(long)clamp_int(heads[0], 0, n - 1) * K + k];
        for (int p = 1; p < nh; ++p) {
          const double v = srow[(long)clamp_int(heads[p], 0, n - 1) * K + k];
          best = (v > best || v != v) ? v : best;                   // a NaN stays, as in np.amax
        }
        hi = hi || best > best_hi;
        lo = lo || best < best_lo;
      }
      const int f = (__ballot(hi) != 0ull ? 1 : 0) | (__ballot(lo) != 0ull ? 2 : 0);
      if (lane == 0) flag[wid] = f;
      __syncthreads();
      const int all = flag[0] | flag[1] | flag[2] | flag[3];
      shadowed = (all & 1) != 0 && (all & 2) == 0;
    }
    if (tid == 0) {
      if (shadowed) {
        label[i] = -2;
      } else {
        label[i] = i;
        heads[nh] = i;                                              // nh < n: at most one head per candidate
      }
    }
    if (!shadowed) ++nh;
    __syncthreads();                                                // heads[nh - 1] is visible; first[] and flag[] are free
  }
}

// workspace: heads [n] int32 | merge [n * n] uint8 (used when the caller passes no merge), rounded up to 8 bytes
size_t global_workspace_need(int n) { return ((size_t)n * sizeof(int32_t) + (size_t)n * n + 7) & ~(size_t)7; }

}  // namespace

extern "C" size_t asw_global_clusters_workspace_bytes(int n) {
  if (n < 0 || n > GLOBAL_MAX_ROWS) {
    asw::set_error(ASW_ERR_ARG, "global_clusters_workspace_bytes: n = %d outside 0..%d", n, GLOBAL_MAX_ROWS);
    return 0;
  }
  return global_workspace_need(n);
}

extern "C" int asw_global_clusters(const double* full, const double* seg, const int32_t* counts, const uint8_t* near, int n,
                                   int K, double sim_db, double win_hi, double win_lo, double best_hi, double best_lo,
                                   void* workspace, size_t workspace_bytes, int32_t* label, uint8_t* merge, void* stream) {
  ASW_CHECK_ARG(n >= 0 && n <= GLOBAL_MAX_ROWS, "global_clusters: n = %d outside 0..%d", n, GLOBAL_MAX_ROWS);
  ASW_CHECK_ARG(K >= 1, "global_clusters: K = %d < 1", K);
  if (n == 0) return ASW_OK;
  ASW_CHECK_ARG(full && seg && counts && near && workspace, "global_clusters: null pointer");
  ASW_CHECK_ARG(label, "global_clusters: null output");
  const size_t need = global_workspace_need(n);
  ASW_CHECK_ARG(workspace_bytes >= need, "global_clusters: workspace of %zu bytes too small, %zu needed", workspace_bytes, need);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "global_clusters: workspace not 8-byte aligned");

  hipStream_t s = asw::as_stream(stream);
  int32_t* heads = static_cast<int32_t*>(workspace);
  uint8_t* mg = merge ? merge : reinterpret_cast<uint8_t*>(heads + n);
  const long pairs = (long)n * n;
  {
    asw::ProfScope prof(s, "global_merge", 0.0, (double)pairs * K * 8);
    hipLaunchKernelGGL(global_merge_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, full, seg, counts, near, n, K,
                       sim_db, win_hi, win_lo, mg);
    ASW_LAUNCH_CHECK();
  }
  asw::ProfScope prof(s, "global_walk", 0.0, (double)pairs);
  hipLaunchKernelGGL(global_walk_kernel, dim3(1), dim3(256), 0, s, seg, counts, mg, n, K, best_hi, best_lo, heads, label);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

// ===========================================================================
// The coarse stage's decision over a lattice (binary_search_baseline, sep/helpers/local_utils_3d.py:339-388, with the
// survivors mask of Prone_method="DENSE_NMS") as search.coarse_select_f64 states it: one float64 multiply per cube and
// comparisons of exact values, so every output byte below is the statement's.  The cubes are cut into slices of
// COARSE_SLICE; a workgroup never waits for another one: the launches are the only hand-over.
// ===========================================================================
namespace {

constexpr int COARSE_SLICE = 1024;                           // cubes per workgroup of coarse_slice_kernel
constexpr int COARSE_MAX_CAP = 64;
constexpr int COARSE_MAX_N = 1 << 24;
constexpr int COARSE_MAX_PARTS = 256;                        // workgroups of coarse_max_kernel at most
constexpr int COARSE_FOLD = COARSE_MAX_CAP + COARSE_SLICE;   // entries coarse_merge_kernel ranks at a time

__device__ __forceinline__ double coarse_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ bool coarse_not_finite(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000LL) == 0x7ff0000000000000LL;
}

// The running maximum that skips NaN (m = NaN: nothing seen yet).  Of two zeros the positive one stays, so the result
// is a function of the set of values and not of the order they are met in.
__device__ __forceinline__ double coarse_max2(double m, double v) {
  if (v != v) return m;
  if (m != m || v > m) return v;
  if (v == m && __double_as_longlong(v) == 0LL) return v;     // +0.0 over -0.0
  return m;
}

__device__ __forceinline__ double coarse_threshold(double max_wd, double thr1, int relative, double rel) {
  if (!relative || max_wd != max_wd) return thr1;
  const double t = rel * max_wd;
  return t < thr1 ? t : thr1;
}

// cube (pa, ia) comes before cube (pb, ib): descending power, equal powers by index, every NaN last by index
__device__ __forceinline__ bool coarse_before(double pa, int ia, double pb, int ib) {
  const bool na = pa != pa, nb = pb != pb;
  if (na || nb) return na == nb ? ia < ib : nb;
  return pa > pb || (pa == pb && ia < ib);
}

// ---------------------------------------------------------------------------
// coarse_max_kernel (relative threshold only): workgroup b strides over the cubes and stores the maximum of the wd it
// met in part[b]; the 256 thread maxima meet in LDS and thread 0 folds them.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void coarse_max_kernel(const double* __restrict__ energies, const double* __restrict__ dis1,
                                                         int N, double* __restrict__ part) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double m = coarse_nan();
  for (long i = (long)blockIdx.x * 256 + tid; i < N; i += (long)gridDim.x * 256) m = coarse_max2(m, energies[2 * i + 1] * dis1[i]);
  red[tid] = m;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 256; ++t) m = coarse_max2(m, red[t]);
    part[blockIdx.x] = m;
  }
}

// ---------------------------------------------------------------------------
// coarse_slice_kernel: workgroup s owns the cubes s * COARSE_SLICE ..., four per thread.  Thread 0 folds the nparts
// maxima of coarse_max_kernel into the threshold (relative) or takes thr1.  Every thread forms wd, the pass flag and
// its share of (cubes that pass, powers that are not finite, maximum of wd); the powers and the flags go to LDS, and
// thread 0 stores the slice's three totals.  A cube that passes then counts the cubes of the slice that pass and come
// before it -- every thread reads the same LDS word at a time, a broadcast -- and that count is its place: the cubes
// with a place below cap store their index into the slice's list, every place once, and the threads from the count on
// store -1.  So all cap slots of the list are written, by plain stores, in an order that does not matter.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void coarse_slice_kernel(const double* __restrict__ energies, const double* __restrict__ dis1,
                                                           const int* __restrict__ best, int N, double thr1, int relative,
                                                           double rel, int cap, const double* __restrict__ part, int nparts,
                                                           double* __restrict__ slice_max, int* __restrict__ slice_cnt,
                                                           int* __restrict__ slice_list) {
  __shared__ double pw[COARSE_SLICE];
  __shared__ unsigned char ok[COARSE_SLICE];
  __shared__ double red[256];
  __shared__ int cnt[256], bad[256];
  __shared__ double thr_s;
  __shared__ int total_s;
  const int tid = threadIdx.x;
  const int base = blockIdx.x * COARSE_SLICE;
  const int len = N - base < COARSE_SLICE ? N - base : COARSE_SLICE;
  if (tid == 0) {
    double m = coarse_nan();
    if (relative)
      for (int p = 0; p < nparts; ++p) m = coarse_max2(m, part[p]);
    thr_s = coarse_threshold(m, thr1, relative, rel);
  }
  __syncthreads();
  const double thr = thr_s;
  double m = coarse_nan();
  int c = 0, b = 0;
#pragma unroll
  for (int k = 0; k < COARSE_SLICE / 256; ++k) {
    const int l = tid + 256 * k, i = base + l;
    double p = 0.0;
    bool pass = false;
    if (l < len) {
      p = energies[2 * (long)i + 1];
      const double wd = p * dis1[i];
      m = coarse_max2(m, wd);
      b += coarse_not_finite(p) ? 1 : 0;
      pass = !(wd < thr) && (best == nullptr || best[i] == i);
      c += pass ? 1 : 0;
    }
    pw[l] = p;
    ok[l] = pass ? 1 : 0;
  }
  red[tid] = m;
  cnt[tid] = c;
  bad[tid] = b;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 256; ++t) {
      m = coarse_max2(m, red[t]);
      c += cnt[t];
      b += bad[t];
    }
    slice_max[blockIdx.x] = m;
    slice_cnt[2 * blockIdx.x] = c;
    slice_cnt[2 * blockIdx.x + 1] = b;
    total_s = c;
  }
  int* __restrict__ list = slice_list + (long)blockIdx.x * cap;
#pragma unroll
  for (int k = 0; k < COARSE_SLICE / 256; ++k) {
    const int l = tid + 256 * k;
    if (!ok[l]) continue;
    const double p = pw[l];
    int r = 0;
    for (int j = 0; j < len; ++j) r += (ok[j] && coarse_before(pw[j], j, p, l)) ? 1 : 0;
    if (r < cap) list[r] = base + l;
  }
  __syncthreads();                                                  // total_s is visible
  if (tid < cap && tid >= total_s) list[tid] = -1;
}

// ---------------------------------------------------------------------------
// coarse_merge_kernel: one workgroup.  It sums the slices' counts, folds their maxima into max_wd and the threshold and
// stores counts[] and thr[].  The best list lives in LDS slots 0 .. 63 (index -1: empty).  The slices' lists are one
// table of nslices * cap entries; COARSE_SLICE of them at a time join the best list in LDS with their powers, read
// again from `energies`, every entry counts the entries that come before it, and those with a place below cap become
// the new best list.  An index outside 0 .. N - 1 is an empty entry.  Four barriers a round: the round's entries are
// loaded; every thread holds its entries' places in registers; the best list is cleared; the new one is written.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void coarse_merge_kernel(const double* __restrict__ energies, int N, double thr1, int relative,
                                                           double rel, int cap, int nslices, const double* __restrict__ slice_max,
                                                           const int* __restrict__ slice_cnt, const int* __restrict__ slice_list,
                                                           int* __restrict__ kept, int* __restrict__ counts,
                                                           double* __restrict__ thr) {
  __shared__ double pw[COARSE_FOLD];
  __shared__ int id[COARSE_FOLD];
  __shared__ double red[256];
  __shared__ int cnt[256], bad[256];
  constexpr int PER = (COARSE_FOLD + 255) / 256;
  const int tid = threadIdx.x;
  {
    double m = coarse_nan();
    int c = 0, b = 0;
    for (int s = tid; s < nslices; s += 256) {
      m = coarse_max2(m, slice_max[s]);
      c += slice_cnt[2 * s];
      b += slice_cnt[2 * s + 1];
    }
    red[tid] = m;
    cnt[tid] = c;
    bad[tid] = b;
    __syncthreads();
    if (tid == 0) {
      for (int t = 1; t < 256; ++t) {
        m = coarse_max2(m, red[t]);
        c += cnt[t];
        b += bad[t];
      }
      counts[0] = c;
      counts[1] = b;
      thr[0] = coarse_threshold(m, thr1, relative, rel);
      thr[1] = m;
    }
  }
  if (tid < COARSE_MAX_CAP) {
    id[tid] = -1;
    pw[tid] = 0.0;
  }
  const long M = (long)nslices * cap;
  for (long c0 = 0; c0 < M; c0 += COARSE_SLICE) {
#pragma unroll
    for (int k = 0; k < COARSE_SLICE / 256; ++k) {
      const int l = tid + 256 * k;
      int v = -1;
      double p = 0.0;
      if (c0 + l < M) {
        v = slice_list[c0 + l];
        if (v < 0 || v >= N) v = -1;
        if (v >= 0) p = energies[2 * (long)v + 1];
      }
      id[COARSE_MAX_CAP + l] = v;
      pw[COARSE_MAX_CAP + l] = p;
    }
    __syncthreads();
    int my_id[PER], my_r[PER];
    double my_p[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int e = tid + 256 * k;
      my_id[k] = e < COARSE_FOLD ? id[e] : -1;
      my_p[k] = e < COARSE_FOLD ? pw[e] : 0.0;
      my_r[k] = 0;
    }
    for (int j = 0; j < COARSE_FOLD; ++j) {
      const int ij = id[j];
      if (ij < 0) continue;                                         // the same word for every thread: a uniform branch
      const double pj = pw[j];
#pragma unroll
      for (int k = 0; k < PER; ++k) my_r[k] += (my_id[k] >= 0 && coarse_before(pj, ij, my_p[k], my_id[k])) ? 1 : 0;
    }
    __syncthreads();
    if (tid < COARSE_MAX_CAP) id[tid] = -1;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (my_id[k] >= 0 && my_r[k] < cap) {
        id[my_r[k]] = my_id[k];
        pw[my_r[k]] = my_p[k];
      }
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid < cap) kept[tid] = id[tid];
}

// workspace: part [COARSE_MAX_PARTS] float64 | slice_max [ns] float64 | slice_cnt [ns][2] int32 | slice_list [ns][cap]
// int32, ns = the number of slices; rounded up to 8 bytes
size_t coarse_slices(int N) { return ((size_t)N + COARSE_SLICE - 1) / COARSE_SLICE; }
size_t coarse_workspace_need(int N, int cap) {
  const size_t ns = coarse_slices(N);
  return (((size_t)COARSE_MAX_PARTS + ns) * sizeof(double) + ns * (2 + (size_t)cap) * sizeof(int32_t) + 7) & ~(size_t)7;
}

}  // namespace

extern "C" size_t asw_coarse_select_workspace_bytes(int N, int cap) {
  if (N < 0 || N > COARSE_MAX_N || cap < 1 || cap > COARSE_MAX_CAP) {
    asw::set_error(ASW_ERR_ARG, "coarse_select_workspace_bytes: N = %d outside 0..%d or cap = %d outside 1..%d", N, COARSE_MAX_N,
                   cap, COARSE_MAX_CAP);
    return 0;
  }
  return coarse_workspace_need(N, cap);
}

extern "C" int asw_coarse_select(const double* energies, const double* dis1, const int32_t* best, int N, double thr1,
                                 int relative, double rel, int cap, void* workspace, size_t workspace_bytes, int32_t* kept,
                                 int32_t* counts, double* thr, void* stream) {
  ASW_CHECK_ARG(N >= 0 && N <= COARSE_MAX_N, "coarse_select: N = %d outside 0..%d", N, COARSE_MAX_N);
  ASW_CHECK_ARG(cap >= 1 && cap <= COARSE_MAX_CAP, "coarse_select: cap = %d outside 1..%d", cap, COARSE_MAX_CAP);
  ASW_CHECK_ARG(kept && counts && thr, "coarse_select: null output");
  hipStream_t s = asw::as_stream(stream);
  if (N == 0) {
    // no cube: nothing to launch; the outputs are (-1 ..), (0, 0), (thr1, NaN), written as 32-bit words
    uint64_t bits[2] = {0, 0x7ff8000000000000ULL};
    memcpy(&bits[0], &thr1, sizeof(double));
    ASW_HIP(hipMemsetAsync(kept, 0xff, (size_t)cap * sizeof(int32_t), s));
    ASW_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s));
    for (int w = 0; w < 4; ++w)
      ASW_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reinterpret_cast<uint32_t*>(thr) + w),
                                (int)(uint32_t)(bits[w / 2] >> (32 * (w & 1))), 1, s));
    return ASW_OK;
  }
  ASW_CHECK_ARG(energies && dis1 && workspace, "coarse_select: null pointer");
  const size_t need = coarse_workspace_need(N, cap);
  ASW_CHECK_ARG(workspace_bytes >= need, "coarse_select: workspace of %zu bytes too small, %zu needed", workspace_bytes, need);
  ASW_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "coarse_select: workspace not 8-byte aligned");

  const int ns = (int)coarse_slices(N);
  double* part = static_cast<double*>(workspace);
  double* slice_max = part + COARSE_MAX_PARTS;
  int32_t* slice_cnt = reinterpret_cast<int32_t*>(slice_max + ns);
  int32_t* slice_list = slice_cnt + 2 * (size_t)ns;
  const int nparts = ns < COARSE_MAX_PARTS ? ns : COARSE_MAX_PARTS;
  if (relative) {
    asw::ProfScope prof(s, "coarse_max", 0.0, (double)N * 24);
    hipLaunchKernelGGL(coarse_max_kernel, dim3(nparts), dim3(256), 0, s, energies, dis1, N, part);
    ASW_LAUNCH_CHECK();
  }
  {
    asw::ProfScope prof(s, "coarse_slices", 0.0, (double)N * 28);
    hipLaunchKernelGGL(coarse_slice_kernel, dim3(ns), dim3(256), 0, s, energies, dis1, best, N, thr1, relative ? 1 : 0, rel, cap,
                       part, nparts, slice_max, slice_cnt, slice_list);
    ASW_LAUNCH_CHECK();
  }
  asw::ProfScope prof(s, "coarse_merge", 0.0, (double)ns * (cap + 2) * 4);
  hipLaunchKernelGGL(coarse_merge_kernel, dim3(1), dim3(256), 0, s, energies, N, thr1, relative ? 1 : 0, rel, cap, ns, slice_max,
                     slice_cnt, slice_list, kept, counts, thr);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
