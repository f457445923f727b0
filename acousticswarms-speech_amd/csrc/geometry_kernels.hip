// geometry_kernels.hip -- the one-off geometry tables of the SRP-PHAT stage built on the device.
//
// Replaces the host build of SRPPhat (srp.py: _lookup_grid, _valid_mask, _map_3d_tdoa and the tau / tops_delta /
// dis_matrix statements; reference: SRP_PHAT.__init__, Map_3D_TDoA and search_cluster,
// sep/Traditional_SP/SRP_Prunning.py:149-180,277-344,368-381) for arrays that change per mixture:
//   lookup_planes   pair-major TDoA tables planes[P][ny][nx][nz] of the 5 cm / 1 cm lookup grids
//   voxel_map       quantised TDoA vector and keep-out mask per voxel of the SRP grid, dis_matrix
//   label           26-connected components of equal quantised vectors, label = smallest C-order voxel index
//   compact         POWER_INDEX, cluster offsets, CSR member list, cluster centres, tau and tops_delta
//   lattice         the coarse TDoA lattice of the 1 cm lookup grid (dense_grid.coarse_lattice): stage 1 without a pruner
//   lattice_nms     local maxima of scores over that lattice (dense_grid.lattice_local_maxima): Prone_method="DENSE_NMS"
//
// Exactness.  Every value is computed in double with the expression order of the numpy statements it
// replaces -- norm = sqrt((dx*dx + dy*dy) + dz*dz), "/ C * FS" as two operations, centres as a sequential sum in
// member order divided by the count -- with IEEE sqrt and divide and with contraction off for the whole file, so
// no fma changes a rounding.  Nothing here accumulates through atomics and the sort is a stable radix sort: two
// builds of one geometry are bit-identical.
#pragma clang fp contract(off)
#include <hipcub/hipcub.hpp>

#include "asw_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxVoxels = 1 << 24;          // labels and CSR indices are int32
constexpr int kLabelBurst = 4;               // propagation sweeps between two reads of the "changed" flag

// |p - m| in numpy.linalg.norm's order for a length-3 axis: (s0 + s1) + s2
__device__ __forceinline__ double norm3(double dx, double dy, double dz) {
  return __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
}

// thread = one lookup point ((y*nx + x)*nz + z); planes[p][point] = (|pt - m_{p+1}| - |pt - m_0|) / C * FS
__global__ __launch_bounds__(kBlock) void lookup_planes_kernel(const double* __restrict__ ys, int ny,
                                                               const double* __restrict__ xs, int nx,
                                                               const double* __restrict__ zs, int nz,
                                                               const double* __restrict__ mics, int M, double C, double FS,
                                                               double* __restrict__ planes) {
  const long total = (long)ny * nx * nz;
  const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int z = (int)(idx % nz);
  const long yx = idx / nz;
  const int x = (int)(yx % nx), y = (int)(yx / nx);
  const double px = xs[x], py = ys[y], pz = zs[z];
  const double d0 = norm3(px - mics[0], py - mics[1], pz - mics[2]) / C * FS;
  for (int i = 1; i < M; ++i) {
    const double d = norm3(px - mics[3 * i], py - mics[3 * i + 1], pz - mics[3 * i + 2]) / C * FS;
    planes[(long)(i - 1) * total + idx] = d - d0;
  }
}

// thread = one voxel (ix*Ly + iy)*Lz + iz.  q[v][p] = rint(((d_{p+1} - d_0) / C * FS) / res) * res (rint rounds
// half to even, as numpy.round does); valid = outside the keep-out rectangle around the array (open interval).
__global__ __launch_bounds__(kBlock) void voxel_map_kernel(const double* __restrict__ xs, int Lx,
                                                           const double* __restrict__ ys, int Ly,
                                                           const double* __restrict__ zs, int Lz,
                                                           const double* __restrict__ mics, int M, double b0, double b1,
                                                           double b2, double b3, double C, double FS, double res,
                                                           int32_t* __restrict__ q, uint8_t* __restrict__ valid) {
  const int n = Lx * Ly * Lz;
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const int iz = v % Lz, iy = (v / Lz) % Ly, ix = v / (Lz * Ly);
  const double px = xs[ix], py = ys[iy], pz = zs[iz];
  const double d0 = norm3(px - mics[0], py - mics[1], pz - mics[2]);
  const int ires = (int)res;
  for (int i = 1; i < M; ++i) {
    const double d = norm3(px - mics[3 * i], py - mics[3 * i + 1], pz - mics[3 * i + 2]);
    const double off = (d - d0) / C * FS;
    q[(long)v * (M - 1) + (i - 1)] = (int32_t)rint(off / res) * ires;
  }
  const bool inside = px > b0 && px < b2 && py > b1 && py < b3;
  valid[v] = inside ? 0 : 1;
}

// thread = one (ix, iy): sqrt((x - cx)^2 + (y - cy)^2) + 1e-8
__global__ __launch_bounds__(kBlock) void dis_matrix_kernel(const double* __restrict__ xs, int Lx,
                                                            const double* __restrict__ ys, int Ly, double cx, double cy,
                                                            double* __restrict__ dis) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= Lx * Ly) return;
  const double a = xs[i / Ly] - cx, b = ys[i % Ly] - cy;
  dis[i] = __dsqrt_rn(a * a + b * b) + 1e-8;
}

// Neighbour k of 27 is (k/9 - 1, (k/3)%3 - 1, k%3 - 1).  adj bit k: that neighbour exists, is valid and has the same
// quantised vector.  labels start at the voxel's own index (-1: invalid voxel).
__global__ __launch_bounds__(kBlock) void label_init_kernel(const int32_t* __restrict__ q, const uint8_t* __restrict__ valid,
                                                            int Lx, int Ly, int Lz, int P, uint32_t* __restrict__ adj,
                                                            int32_t* __restrict__ labels) {
  const int n = Lx * Ly * Lz;
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  if (!valid[v]) {
    adj[v] = 0;
    labels[v] = -1;
    return;
  }
  const int iz = v % Lz, iy = (v / Lz) % Ly, ix = v / (Lz * Ly);
  uint32_t bits = 0;
  for (int k = 0; k < 27; ++k) {
    if (k == 13) continue;
    const int jx = ix + k / 9 - 1, jy = iy + (k / 3) % 3 - 1, jz = iz + k % 3 - 1;
    if (jx < 0 || jx >= Lx || jy < 0 || jy >= Ly || jz < 0 || jz >= Lz) continue;
    const int u = (jx * Ly + jy) * Lz + jz;
    if (!valid[u]) continue;
    bool same = true;
    for (int p = 0; p < P; ++p) same = same && q[(long)u * P + p] == q[(long)v * P + p];
    if (same) bits |= 1u << k;
  }
  adj[v] = bits;
  labels[v] = v;
}

// One sweep of min-label propagation with a pointer jump.  A voxel's label is written by its own thread only, always
// with a smaller index of its own component, so the sweeps may read labels other threads are lowering: whatever they
// see, the fixed point -- every voxel carrying the smallest index of its component -- is the same.
__global__ __launch_bounds__(kBlock) void label_sweep_kernel(const uint32_t* __restrict__ adj, int Lx, int Ly, int Lz,
                                                             volatile int32_t* labels, int32_t* __restrict__ changed) {
  const int n = Lx * Ly * Lz;
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const int32_t cur = labels[v];
  if (cur < 0) return;
  const uint32_t bits = adj[v];
  int32_t best = cur;
  for (int k = 0; k < 27; ++k) {
    if (!((bits >> k) & 1u)) continue;
    const int u = v + ((k / 9 - 1) * Ly + ((k / 3) % 3 - 1)) * Lz + (k % 3 - 1);
    const int32_t l = labels[u];
    best = l < best ? l : best;
  }
  const int32_t up = labels[best];           // best is a voxel of this component, its label another one, not larger
  best = up < best ? up : best;
  if (best < cur) {
    labels[v] = best;
    *changed = 1;
  }
}

__global__ __launch_bounds__(kBlock) void flags_kernel(const int32_t* __restrict__ labels, int n, int32_t* __restrict__ rootf,
                                                       int32_t* __restrict__ validf) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const int32_t l = labels[v];
  rootf[v] = l == v ? 1 : 0;
  validf[v] = l >= 0 ? 1 : 0;
}

// rank = exclusive scan of the root flags: the component whose smallest voxel comes first in C order is cluster 0,
// which is the order the reference's (ix, iy, iz) scan meets them in.
__global__ __launch_bounds__(kBlock) void scatter_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ q, int n,
                                                         int P, const int32_t* __restrict__ rank,
                                                         const int32_t* __restrict__ vpos, int32_t* __restrict__ power_index,
                                                         int32_t* __restrict__ valid_flat, int32_t* __restrict__ valid_cid,
                                                         int32_t* __restrict__ offsets) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  const int32_t l = labels[v];
  if (l < 0 || l >= n) {                      // invalid voxel (a label outside the lattice cannot index rank[])
    power_index[v] = 0;
    return;
  }
  const int32_t cid = rank[l];
  power_index[v] = cid;
  const int32_t j = vpos[v];
  valid_flat[j] = v;
  valid_cid[j] = cid;
  if (l == v)
    for (int p = 0; p < P; ++p) offsets[(long)cid * P + p] = q[(long)v * P + p];
}

// bounds[g] = first position of cluster g in the sorted keys (g = G gives V)
__global__ __launch_bounds__(kBlock) void bounds_kernel(const int32_t* __restrict__ keys, int V, int G, int32_t* __restrict__ bounds) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g > G) return;
  int lo = 0, hi = V;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < g) lo = mid + 1; else hi = mid;
  }
  bounds[g] = lo;
}

// thread = one cluster: its members' positions summed one after the other in ascending voxel index, then / count
__global__ __launch_bounds__(kBlock) void centres_kernel(const int32_t* __restrict__ members, const int32_t* __restrict__ bounds,
                                                         int G, const double* __restrict__ xs, const double* __restrict__ ys,
                                                         const double* __restrict__ zs, int Ly, int Lz,
                                                         double* __restrict__ centres) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= G) return;
  const int b0 = bounds[g], b1 = bounds[g + 1];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = b0; j < b1; ++j) {
    const int v = members[j];
    const double px = xs[v / (Lz * Ly)], py = ys[(v / Lz) % Ly], pz = zs[v % Lz];
    if (j == b0) {
      sx = px; sy = py; sz = pz;
    } else {
      sx = sx + px; sy = sy + py; sz = sz + pz;
    }
  }
  const double cnt = (double)(b1 - b0);
  centres[3 * (long)g] = sx / cnt;
  centres[3 * (long)g + 1] = sy / cnt;
  centres[3 * (long)g + 2] = sz / cnt;
}

// thread = one (cluster, mic).  tau ignores the mic's z and takes the point's z absolute (generate_mod_vector);
// delta = |p - c| - |(p - c) - (m - c)| with c the mic mean (TOPS_block.py:45-48,105-112).
__global__ __launch_bounds__(kBlock) void delays_kernel(const double* __restrict__ centres, int G, const double* __restrict__ mics,
                                                        int M, double cx, double cy, double cz, double C,
                                                        double* __restrict__ tau, double* __restrict__ delta) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long)G * M) return;
  const int g = (int)(i / M), m = (int)(i % M);
  const double gx = centres[3 * (long)g], gy = centres[3 * (long)g + 1], gz = centres[3 * (long)g + 2];
  const double mx = mics[3 * m], my = mics[3 * m + 1], mz = mics[3 * m + 2];
  const double dx = gx - mx, dy = gy - my;
  tau[i] = __dsqrt_rn((dx * dx + dy * dy) + gz * gz) / C;
  const double px = gx - cx, py = gy - cy, pz = gz - cz;
  const double ex = px - (mx - cx), ey = py - (my - cy), ez = pz - (mz - cz);
  delta[i] = norm3(px, py, pz) - norm3(ex, ey, ez);
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int sort_bits(int G) {
  int bits = 1;
  while (bits < 31 && (1 << bits) < G) ++bits;
  return bits;
}

// temporary storage of the scans and of the radix sort over n items (the larger of the two)
hipError_t cub_temp_bytes(int n, size_t* bytes) {
  size_t a = 0, b = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const int32_t*)nullptr, (int32_t*)nullptr, n, (hipStream_t)0);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr,
                                         (int32_t*)nullptr, n, 0, 32, (hipStream_t)0);
  *bytes = a > b ? a : b;
  return e;
}

bool good_axes(int a, int b, int c) {
  return a > 0 && b > 0 && c > 0 && (long)a * b * c <= kMaxVoxels;
}

}  // namespace

extern "C" int asw_geom_lookup_planes(const double* ys, int ny, const double* xs, int nx, const double* zs, int nz,
                                      const double* mics, int M, double C, double FS, double* planes, void* stream) {
  ASW_CHECK_ARG(ys && xs && zs && mics && planes, "geom_lookup_planes: null pointer");
  ASW_CHECK_ARG(ny > 0 && nx > 0 && nz > 0 && (long)ny * nx * nz <= 0x7fffffffL,
                "geom_lookup_planes: bad grid %d x %d x %d (the cube scans index points with int32)", ny, nx, nz);
  ASW_CHECK_ARG(M >= 2 && M <= 32, "geom_lookup_planes: M = %d outside 2..32", M);
  ASW_CHECK_ARG(C > 0 && FS > 0, "geom_lookup_planes: C and FS must be positive");
  const long total = (long)ny * nx * nz;
  hipLaunchKernelGGL(lookup_planes_kernel, dim3(asw::cdiv(total, kBlock)), dim3(kBlock), 0, asw::as_stream(stream), ys, ny, xs,
                     nx, zs, nz, mics, M, C, FS, planes);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" int asw_geom_voxel_map(const double* xs, int Lx, const double* ys, int Ly, const double* zs, int Lz,
                                  const double* mics, int M, const double* border, const double* centre, double C, double FS,
                                  double resolution, int32_t* q, uint8_t* valid, double* dis_matrix, void* stream) {
  ASW_CHECK_ARG(xs && ys && zs && mics && border && centre && q && valid && dis_matrix, "geom_voxel_map: null pointer");
  ASW_CHECK_ARG(good_axes(Lx, Ly, Lz), "geom_voxel_map: bad lattice %d x %d x %d", Lx, Ly, Lz);
  ASW_CHECK_ARG(M >= 2 && M <= 32, "geom_voxel_map: M = %d outside 2..32", M);
  ASW_CHECK_ARG(C > 0 && FS > 0, "geom_voxel_map: C and FS must be positive");
  ASW_CHECK_ARG(resolution >= 1 && resolution <= 1024 && resolution == (double)(int)resolution,
                "geom_voxel_map: the sample resolution must be a whole number of samples in 1..1024");
  hipStream_t s = asw::as_stream(stream);
  const int n = Lx * Ly * Lz;
  hipLaunchKernelGGL(voxel_map_kernel, dim3(asw::cdiv(n, kBlock)), dim3(kBlock), 0, s, xs, Lx, ys, Ly, zs, Lz, mics, M, border[0],
                     border[1], border[2], border[3], C, FS, resolution, q, valid);
  ASW_LAUNCH_CHECK();
  hipLaunchKernelGGL(dis_matrix_kernel, dim3(asw::cdiv((long)Lx * Ly, kBlock)), dim3(kBlock), 0, s, xs, Lx, ys, Ly, centre[0],
                     centre[1], dis_matrix);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" int asw_geom_label(const int32_t* q, const uint8_t* valid, int Lx, int Ly, int Lz, int P, uint32_t* adj_scratch,
                              int32_t* flag_scratch, int32_t* labels, int* sweeps, void* stream) {
  ASW_CHECK_ARG(q && valid && adj_scratch && flag_scratch && labels, "geom_label: null pointer");
  ASW_CHECK_ARG(good_axes(Lx, Ly, Lz), "geom_label: bad lattice %d x %d x %d", Lx, Ly, Lz);
  ASW_CHECK_ARG(P >= 1 && P <= 31, "geom_label: P = %d outside 1..31", P);
  hipStream_t s = asw::as_stream(stream);
  const int n = Lx * Ly * Lz, blocks = asw::cdiv(n, kBlock);
  hipLaunchKernelGGL(label_init_kernel, dim3(blocks), dim3(kBlock), 0, s, q, valid, Lx, Ly, Lz, P, adj_scratch, labels);
  ASW_LAUNCH_CHECK();
  int done = 0;
  // a label falls at least once per sweep until the fixed point, so n sweeps are an upper bound no lattice reaches
  for (long it = 0; it < (long)n + kLabelBurst; it += kLabelBurst) {
    ASW_HIP(hipMemsetAsync(flag_scratch, 0, sizeof(int32_t), s));
    for (int k = 0; k < kLabelBurst; ++k) {
      hipLaunchKernelGGL(label_sweep_kernel, dim3(blocks), dim3(kBlock), 0, s, adj_scratch, Lx, Ly, Lz, labels, flag_scratch);
      ASW_LAUNCH_CHECK();
    }
    done += kLabelBurst;
    int32_t changed = 0;
    ASW_HIP(hipMemcpyAsync(&changed, flag_scratch, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ASW_HIP(hipStreamSynchronize(s));
    if (!changed) {
      if (sweeps) *sweeps = done;
      return ASW_OK;
    }
  }
  return asw::set_error(ASW_ERR_STATE, "geom_label: the labels did not settle within %d sweeps", done);
}

extern "C" int64_t asw_geom_workspace_bytes(int n_voxels) {
  if (n_voxels <= 0 || n_voxels > kMaxVoxels) {
    asw::set_error(ASW_ERR_ARG, "geom_workspace_bytes: %d voxels outside 1..%d", n_voxels, kMaxVoxels);
    return ASW_ERR_ARG;
  }
  size_t temp = 0;
  if (cub_temp_bytes(n_voxels, &temp) != hipSuccess) {
    asw::set_error(ASW_ERR_HIP, "geom_workspace_bytes: the scan / sort size query failed");
    return ASW_ERR_HIP;
  }
  return (int64_t)(5 * align256((size_t)n_voxels * sizeof(int32_t)) + align256(temp));
}

extern "C" int asw_geom_compact(const int32_t* labels, const int32_t* q, const double* xs, int Lx, const double* ys, int Ly,
                                const double* zs, int Lz, const double* mics, int M, const double* centre, double C,
                                void* workspace, int64_t workspace_bytes, int32_t* power_index, int32_t* valid_flat,
                                int32_t* valid_cid, int32_t* members, int32_t* bounds, int32_t* offsets, double* centres,
                                double* tau, double* delta, int* counts, void* stream) {
  ASW_CHECK_ARG(labels && q && xs && ys && zs && mics && centre && workspace && counts, "geom_compact: null pointer");
  ASW_CHECK_ARG(power_index && valid_flat && valid_cid && members && bounds && offsets && centres && tau && delta,
                "geom_compact: null output pointer");
  ASW_CHECK_ARG(good_axes(Lx, Ly, Lz), "geom_compact: bad lattice %d x %d x %d", Lx, Ly, Lz);
  ASW_CHECK_ARG(M >= 2 && M <= 32, "geom_compact: M = %d outside 2..32", M);
  ASW_CHECK_ARG(C > 0, "geom_compact: C must be positive");
  const int n = Lx * Ly * Lz, P = M - 1, blocks = asw::cdiv(n, kBlock);
  const size_t slot = align256((size_t)n * sizeof(int32_t));
  ASW_CHECK_ARG(workspace_bytes >= (int64_t)(5 * slot), "geom_compact: workspace of %lld bytes is too small (asw_geom_workspace_bytes)",
                (long long)workspace_bytes);
  size_t temp = (size_t)workspace_bytes - 5 * slot;
  hipStream_t s = asw::as_stream(stream);
  size_t need = 0;
  ASW_HIP(cub_temp_bytes(n, &need));
  ASW_CHECK_ARG(temp >= need, "geom_compact: workspace of %lld bytes is too small (asw_geom_workspace_bytes)",
                (long long)workspace_bytes);
  char* base = static_cast<char*>(workspace);
  int32_t* rootf = reinterpret_cast<int32_t*>(base);
  int32_t* validf = reinterpret_cast<int32_t*>(base + slot);
  int32_t* rank = reinterpret_cast<int32_t*>(base + 2 * slot);
  int32_t* vpos = reinterpret_cast<int32_t*>(base + 3 * slot);
  int32_t* keys = reinterpret_cast<int32_t*>(base + 4 * slot);
  void* cub = base + 5 * slot;

  hipLaunchKernelGGL(flags_kernel, dim3(blocks), dim3(kBlock), 0, s, labels, n, rootf, validf);
  ASW_LAUNCH_CHECK();
  size_t t = temp;
  ASW_HIP(hipcub::DeviceScan::ExclusiveSum(cub, t, rootf, rank, n, s));
  t = temp;
  ASW_HIP(hipcub::DeviceScan::ExclusiveSum(cub, t, validf, vpos, n, s));
  hipLaunchKernelGGL(scatter_kernel, dim3(blocks), dim3(kBlock), 0, s, labels, q, n, P, rank, vpos, power_index, valid_flat,
                     valid_cid, offsets);
  ASW_LAUNCH_CHECK();
  int32_t last[4] = {0, 0, 0, 0};
  ASW_HIP(hipMemcpyAsync(&last[0], rank + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ASW_HIP(hipMemcpyAsync(&last[1], rootf + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ASW_HIP(hipMemcpyAsync(&last[2], vpos + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ASW_HIP(hipMemcpyAsync(&last[3], validf + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ASW_HIP(hipStreamSynchronize(s));
  const int G = last[0] + last[1], V = last[2] + last[3];
  counts[0] = G;
  counts[1] = V;
  if (G < 0 || V < G || V > n) return asw::set_error(ASW_ERR_STATE, "geom_compact: inconsistent labels (G = %d, V = %d, n = %d)", G, V, n);
  if (G == 0) return ASW_OK;
  t = temp;
  ASW_HIP(hipcub::DeviceRadixSort::SortPairs(cub, t, valid_cid, keys, valid_flat, members, V, 0, sort_bits(G), s));
  hipLaunchKernelGGL(bounds_kernel, dim3(asw::cdiv(G + 1, kBlock)), dim3(kBlock), 0, s, keys, V, G, bounds);
  ASW_LAUNCH_CHECK();
  hipLaunchKernelGGL(centres_kernel, dim3(asw::cdiv(G, kBlock)), dim3(kBlock), 0, s, members, bounds, G, xs, ys, zs, Ly, Lz, centres);
  ASW_LAUNCH_CHECK();
  hipLaunchKernelGGL(delays_kernel, dim3(asw::cdiv((long)G * M, kBlock)), dim3(kBlock), 0, s, centres, G, mics, M, centre[0],
                     centre[1], centre[2], C, tau, delta);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

// ---- coarse TDoA lattice of the 1 cm lookup grid (dense_grid.coarse_lattice) -------------------------------------
// Every lookup point outside the keep-out rectangle belongs to the cube its TDoA vector rounds to; the cubes come out
// in lexicographic order of their cell vectors and the members of a cube in ascending point index.  The cell vector
// of 16 microphones is 15 int32 fields (up to 31): it is ordered by one stable radix pass per pair, last pair first.
namespace {

// thread = one lookup point i = (iy*nx + ix)*nz + iz: keep[i] = outside the keep-out rectangle (open interval, the
// comparisons of SRPPhat._valid_mask), cellp[p][i] = rint(planes[p][i] / width) (IEEE divide, round half to even)
__global__ __launch_bounds__(kBlock) void lattice_cells_kernel(const double* __restrict__ planes, int P, long n, int nx, int nz,
                                                               const double* __restrict__ xs, const double* __restrict__ ys,
                                                               double b0, double b1, double b2, double b3, double width,
                                                               int32_t* __restrict__ cellp, int32_t* __restrict__ keep) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const long yx = i / nz;
  const double px = xs[yx % nx], py = ys[yx / nx];
  const bool inside = px > b0 && px < b2 && py > b1 && py < b3;
  keep[i] = inside ? 0 : 1;
  for (int p = 0; p < P; ++p) cellp[(long)p * n + i] = (int32_t)rint(planes[(long)p * n + i] / width);
}

// kept points in ascending index: perm[pos[i]] = i
__global__ __launch_bounds__(kBlock) void lattice_compact_kernel(const int32_t* __restrict__ keep, const int32_t* __restrict__ pos,
                                                                 long n, int32_t* __restrict__ perm) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (keep[i]) perm[pos[i]] = (int32_t)i;
}

// keys of one radix pass: the cell of pair p of the points in their current order
__global__ __launch_bounds__(kBlock) void lattice_keys_kernel(const int32_t* __restrict__ plane, const int32_t* __restrict__ perm,
                                                              int K, int32_t* __restrict__ keys) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= K) return;
  keys[j] = plane[perm[j]];
}

// head[j] = 1 where sorted point j opens a cube (its cell vector differs from its predecessor's)
__global__ __launch_bounds__(kBlock) void lattice_heads_kernel(const int32_t* __restrict__ cellp, int P, long n,
                                                               const int32_t* __restrict__ perm, int K, int32_t* __restrict__ head) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= K) return;
  int32_t h = 1;
  if (j > 0) {
    const int32_t a = perm[j], b = perm[j - 1];
    h = 0;
    for (int p = 0; p < P; ++p) h |= cellp[(long)p * n + a] != cellp[(long)p * n + b] ? 1 : 0;
  }
  head[j] = h;
}

// rank = exclusive scan of head: a head is cube rank[j]; it writes the cube's first position and cell vector
__global__ __launch_bounds__(kBlock) void lattice_scatter_kernel(const int32_t* __restrict__ cellp, int P, long n,
                                                                 const int32_t* __restrict__ perm, int K,
                                                                 const int32_t* __restrict__ head, const int32_t* __restrict__ rank,
                                                                 int32_t* __restrict__ cells, int32_t* __restrict__ bounds) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= K) return;
  if (head[j]) {
    const int32_t g = rank[j], a = perm[j];
    bounds[g] = j;
    for (int p = 0; p < P; ++p) cells[(long)g * P + p] = cellp[(long)p * n + a];
  }
  if (j == K - 1) bounds[rank[j] + head[j]] = K;
}

// thread = one cube: its members' positions summed one after the other in member order, then / count (centres_kernel
// with the lookup grid's point index)
__global__ __launch_bounds__(kBlock) void lattice_centres_kernel(const int32_t* __restrict__ members, const int32_t* __restrict__ bounds,
                                                                 int N, const double* __restrict__ xs, const double* __restrict__ ys,
                                                                 const double* __restrict__ zs, int nx, int nz,
                                                                 double* __restrict__ centres) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= N) return;
  const int b0 = bounds[g], b1 = bounds[g + 1];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = b0; j < b1; ++j) {
    const int i = members[j];
    const int yx = i / nz;
    const double px = xs[yx % nx], py = ys[yx / nx], pz = zs[i % nz];
    if (j == b0) {
      sx = px; sy = py; sz = pz;
    } else {
      sx = sx + px; sy = sy + py; sz = sz + pz;
    }
  }
  const double cnt = (double)(b1 - b0);
  centres[3 * (long)g] = sx / cnt;
  centres[3 * (long)g + 1] = sy / cnt;
  centres[3 * (long)g + 2] = sz / cnt;
}

constexpr int kLatticeSlots = 6;             // keep / head, pos / rank, two permutations, two key arrays

}  // namespace

extern "C" int64_t asw_geom_lattice_workspace_bytes(int n_points, int P) {
  if (n_points <= 0 || P < 1 || P > 31) {
    asw::set_error(ASW_ERR_ARG, "geom_lattice_workspace_bytes: %d points, %d pairs (need points > 0, 1 <= pairs <= 31)", n_points, P);
    return ASW_ERR_ARG;
  }
  size_t temp = 0;
  if (cub_temp_bytes(n_points, &temp) != hipSuccess) {
    asw::set_error(ASW_ERR_HIP, "geom_lattice_workspace_bytes: the scan / sort size query failed");
    return ASW_ERR_HIP;
  }
  return (int64_t)((size_t)(P + kLatticeSlots) * align256((size_t)n_points * sizeof(int32_t)) + align256(temp));
}

extern "C" int asw_geom_lattice(const double* planes, int P, int ny, int nx, int nz, const double* xs, const double* ys,
                                const double* zs, const double* border, double width, void* workspace, int64_t workspace_bytes,
                                int32_t* cells, int32_t* bounds, int32_t* members, double* centres, int* counts, void* stream) {
  ASW_CHECK_ARG(planes && xs && ys && zs && border && workspace && counts, "geom_lattice: null pointer");
  ASW_CHECK_ARG(cells && bounds && members && centres, "geom_lattice: null output pointer");
  ASW_CHECK_ARG(ny > 0 && nx > 0 && nz > 0 && (long)ny * nx * nz <= 0x7fffffffL,
                "geom_lattice: bad grid %d x %d x %d (points are indexed with int32)", ny, nx, nz);
  ASW_CHECK_ARG(P >= 1 && P <= 31, "geom_lattice: P = %d outside 1..31", P);
  ASW_CHECK_ARG(width >= 1.0 / 1024 && width <= 1024, "geom_lattice: the cube width must lie in 1/1024..1024 samples");
  const long n = (long)ny * nx * nz;
  const size_t slot = align256((size_t)n * sizeof(int32_t));
  const size_t fixed = (size_t)(P + kLatticeSlots) * slot;
  size_t need = 0;
  ASW_HIP(cub_temp_bytes((int)n, &need));
  ASW_CHECK_ARG(workspace_bytes >= (int64_t)(fixed + need),
                "geom_lattice: workspace of %lld bytes is too small (asw_geom_lattice_workspace_bytes)", (long long)workspace_bytes);
  const size_t temp = (size_t)workspace_bytes - fixed;
  hipStream_t s = asw::as_stream(stream);
  char* base = static_cast<char*>(workspace);
  int32_t* cellp = reinterpret_cast<int32_t*>(base);
  char* rest = base + (size_t)P * slot;
  int32_t* keep = reinterpret_cast<int32_t*>(rest);                 // later: head flags of the sorted points
  int32_t* pos = reinterpret_cast<int32_t*>(rest + slot);           // later: their exclusive scan
  int32_t* perm_a = reinterpret_cast<int32_t*>(rest + 2 * slot);
  int32_t* perm_b = reinterpret_cast<int32_t*>(rest + 3 * slot);
  int32_t* keys_a = reinterpret_cast<int32_t*>(rest + 4 * slot);
  int32_t* keys_b = reinterpret_cast<int32_t*>(rest + 5 * slot);
  void* cub = rest + kLatticeSlots * slot;
  const int blocks = asw::cdiv(n, kBlock);

  counts[0] = counts[1] = 0;
  ASW_HIP(hipMemsetAsync(bounds, 0, sizeof(int32_t), s));           // bounds[0] of an empty lattice
  hipLaunchKernelGGL(lattice_cells_kernel, dim3(blocks), dim3(kBlock), 0, s, planes, P, n, nx, nz, xs, ys, border[0], border[1],
                     border[2], border[3], width, cellp, keep);
  ASW_LAUNCH_CHECK();
  size_t t = temp;
  ASW_HIP(hipcub::DeviceScan::ExclusiveSum(cub, t, keep, pos, (int)n, s));
  int32_t last[2] = {0, 0};
  ASW_HIP(hipMemcpyAsync(&last[0], pos + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ASW_HIP(hipMemcpyAsync(&last[1], keep + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ASW_HIP(hipStreamSynchronize(s));
  const int K = last[0] + last[1];
  if (K < 0 || K > n) return asw::set_error(ASW_ERR_STATE, "geom_lattice: inconsistent keep flags (%d kept of %ld points)", K, n);
  counts[1] = K;
  if (K == 0) return ASW_OK;
  hipLaunchKernelGGL(lattice_compact_kernel, dim3(blocks), dim3(kBlock), 0, s, keep, pos, n, perm_a);
  ASW_LAUNCH_CHECK();

  // least significant field first; every pass is stable, so the points end up ordered by the whole cell vector with
  // ties (one cube) left in ascending point index
  const int kblocks = asw::cdiv(K, kBlock);
  int32_t *cur = perm_a, *spare = perm_b;
  for (int p = P - 1; p >= 0; --p) {
    int32_t* out = p == 0 ? members : spare;                        // the last pass leaves the member list in place
    hipLaunchKernelGGL(lattice_keys_kernel, dim3(kblocks), dim3(kBlock), 0, s, cellp + (long)p * n, cur, K, keys_a);
    ASW_LAUNCH_CHECK();
    t = temp;
    ASW_HIP(hipcub::DeviceRadixSort::SortPairs(cub, t, keys_a, keys_b, cur, out, K, 0, 32, s));
    spare = cur;
    cur = out;
  }
  int32_t *head = keep, *rank = pos;
  hipLaunchKernelGGL(lattice_heads_kernel, dim3(kblocks), dim3(kBlock), 0, s, cellp, P, n, members, K, head);
  ASW_LAUNCH_CHECK();
  t = temp;
  ASW_HIP(hipcub::DeviceScan::ExclusiveSum(cub, t, head, rank, K, s));
  hipLaunchKernelGGL(lattice_scatter_kernel, dim3(kblocks), dim3(kBlock), 0, s, cellp, P, n, members, K, head, rank, cells, bounds);
  ASW_LAUNCH_CHECK();
  ASW_HIP(hipMemcpyAsync(&last[0], rank + (K - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ASW_HIP(hipMemcpyAsync(&last[1], head + (K - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ASW_HIP(hipStreamSynchronize(s));
  const int N = last[0] + last[1];
  if (N < 1 || N > K) return asw::set_error(ASW_ERR_STATE, "geom_lattice: inconsistent head flags (N = %d, kept = %d)", N, K);
  counts[0] = N;
  hipLaunchKernelGGL(lattice_centres_kernel, dim3(asw::cdiv(N, kBlock)), dim3(kBlock), 0, s, members, bounds, N, xs, ys, zs, nx, nz,
                     centres);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

// ---- non-maximum suppression over the lattice (dense_grid.lattice_local_maxima) ----------------------------------
// Cube j is near cube i when every pair's cells differ by at most `radius`; best[i] is the near cube with the largest
// score (lowest index among equals), degree[i] the number of near cubes other than i.  An all-pairs test: one thread
// owns cube i (cells and running champion in registers), the cubes j pass by in LDS tiles, and the j range is split
// over gridDim.y so that a few thousand cubes still fill the device.  Integer compares and exact float64 compares
// only, no atomics: a split leaves a partial champion and a partial degree per cube in the workspace (every slot is
// written, so what the workspace held before does not matter) and a second kernel combines them in split order.
namespace {

constexpr int kNmsTile = 256;                // cubes j per LDS tile, and cubes i per block (one per thread)
constexpr int kNmsStride = kNmsTile + 1;     // row stride of the transposed tile: the staging writes spread over the banks
constexpr int kNmsMaxSplits = 32;
constexpr int kNmsMaxCubes = kMaxVoxels;     // int32 indices and int arithmetic on them with room to spare
// LDS per block: cells [PB][kNmsStride] int32 + scores [kNmsTile] float64 + the j range.  For P = 31 (PB = 31) that is
// 31 * 257 * 4 + 256 * 8 + 8 = 33 924 bytes of the CU's 160 KiB: four blocks per CU.

// splits of the j range: enough blocks for 256 CUs several times over, never less than one tile of j per split
int nms_splits(int N) {
  const int rows = asw::cdiv(N, kNmsTile);
  const int want = asw::cdiv(1024, rows > 0 ? rows : 1);
  const int s = want < rows ? want : rows;
  return s < 1 ? 1 : (s > kNmsMaxSplits ? kNmsMaxSplits : s);
}

// |a - b| of two int32 without overflow
__device__ __forceinline__ uint32_t cell_distance(int32_t a, int32_t b) {
  return a >= b ? (uint32_t)a - (uint32_t)b : (uint32_t)b - (uint32_t)a;
}

// block (x, y): cubes i = x * kNmsTile + thread against split y of the cubes j that can be near them.  The table is
// sorted with pair 0 most significant, so the cubes whose pair-0 cell lies within `radius` of the block's are one
// contiguous range [jlo, jhi), found by bisection in column 0; split y takes its share of that range in whole tiles.
// PB >= P is the compile-time bound that keeps the cube's own cells in registers.
template <int PB>
__global__ __launch_bounds__(kNmsTile) void lattice_nms_kernel(const int32_t* __restrict__ cells, int N, int P,
                                                               const double* __restrict__ scores, uint32_t radius,
                                                               int32_t* __restrict__ part_best, int32_t* __restrict__ part_degree) {
  __shared__ int32_t s_cells[PB * kNmsStride];
  __shared__ double s_scores[kNmsTile];
  __shared__ int s_range[2];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * kNmsTile;
  const int i = i0 + t;
  if (t == 0) {
    const int i_last = (i0 + kNmsTile < N ? i0 + kNmsTile : N) - 1;
    const long lo_v = (long)cells[(long)i0 * P] - (long)radius, hi_v = (long)cells[(long)i_last * P] + (long)radius;
    int a = 0, b = N;                                        // first j with cells[j][0] >= lo_v
    while (a < b) {
      const int m = a + (b - a) / 2;
      if ((long)cells[(long)m * P] < lo_v) a = m + 1; else b = m;
    }
    s_range[0] = a;
    b = N;                                                   // first j with cells[j][0] > hi_v
    while (a < b) {
      const int m = a + (b - a) / 2;
      if ((long)cells[(long)m * P] <= hi_v) a = m + 1; else b = m;
    }
    s_range[1] = a;
  }
  __syncthreads();
  const int jlo = s_range[0], jhi = s_range[1];
  const int tiles = (jhi - jlo + kNmsTile - 1) / kNmsTile, ny = (int)gridDim.y;
  const int per = (tiles + ny - 1) / ny * kNmsTile;                  // j per split, whole tiles
  const long jb_l = (long)jlo + (long)blockIdx.y * per;
  const int jbeg = jb_l < jhi ? (int)jb_l : jhi;
  const int jend = jhi - jbeg < per ? jhi : jbeg + per;

  int32_t mine[PB];
#pragma unroll
  for (int p = 0; p < PB; ++p) mine[p] = (i < N && p < P) ? cells[(long)i * P + p] : 0;
  int best = -1, deg = 0;
  double best_sc = 0.0;
  for (int jb = jbeg; jb < jend; jb += kNmsTile) {
    const int cnt = jend - jb < kNmsTile ? jend - jb : kNmsTile;      // rows past the range are neither read nor counted
    __syncthreads();                                                  // the previous tile has been consumed
    for (int e = t; e < cnt * P; e += kNmsTile) {                     // coalesced read of cnt rows, transposed into LDS
      const int row = e / P, p = e - row * P;
      s_cells[p * kNmsStride + row] = cells[(long)jb * P + e];
    }
    if (t < cnt) s_scores[t] = scores[jb + t];
    __syncthreads();
    for (int jj = 0; jj < cnt; ++jj) {                                // every lane reads the same j: LDS broadcasts
      bool near = true;
#pragma unroll
      for (int p = 0; p < PB; ++p)
        if (p < P) near &= cell_distance(mine[p], s_cells[p * kNmsStride + jj]) <= radius;
      const int j = jb + jj;
      const double sc = s_scores[jj];
      deg += (near && j != i) ? 1 : 0;
      if (near && (best < 0 || sc > best_sc)) {                       // j ascends: an equal score keeps the lower index
        best = j;
        best_sc = sc;
      }
    }
  }
  if (i < N) {
    part_best[(long)blockIdx.y * N + i] = best;                       // -1: no near cube in this split
    part_degree[(long)blockIdx.y * N + i] = deg;
  }
}

// thread = one cube: the partial champions in split order (largest score, lowest index among equals), degrees summed
__global__ __launch_bounds__(kBlock) void lattice_nms_combine_kernel(const int32_t* __restrict__ part_best,
                                                                     const int32_t* __restrict__ part_degree,
                                                                     const double* __restrict__ scores, int N, int splits,
                                                                     int32_t* __restrict__ best, int32_t* __restrict__ degree) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  int b = -1, d = 0;
  double bs = 0.0;
  for (int s = 0; s < splits; ++s) {
    const int j = part_best[(long)s * N + i];
    d += part_degree[(long)s * N + i];
    if (j < 0) continue;
    const double sc = scores[j];
    if (b < 0 || sc > bs || (sc == bs && j < b)) {
      b = j;
      bs = sc;
    }
  }
  best[i] = b < 0 ? i : b;                   // a cube is near itself; b < 0 only on a table that breaks the sort order
  degree[i] = d;
}

}  // namespace

extern "C" int64_t asw_lattice_nms_workspace_bytes(int N, int P) {
  if (N < 0 || N > kNmsMaxCubes || P < 1 || P > 31) {
    asw::set_error(ASW_ERR_ARG, "lattice_nms_workspace_bytes: %d cubes, %d pairs (need 0 <= cubes <= %d, 1 <= pairs <= 31)", N, P,
                   kNmsMaxCubes);
    return ASW_ERR_ARG;
  }
  return (int64_t)(2 * align256((size_t)nms_splits(N) * (size_t)N * sizeof(int32_t)));
}

extern "C" int asw_lattice_nms(const int32_t* cells, int N, int P, const double* scores, int radius, void* workspace,
                               int64_t workspace_bytes, int32_t* best, int32_t* degree, void* stream) {
  ASW_CHECK_ARG(N >= 0 && N <= kNmsMaxCubes, "lattice_nms: N = %d outside 0..%d", N, kNmsMaxCubes);
  ASW_CHECK_ARG(P >= 1 && P <= 31, "lattice_nms: P = %d outside 1..31", P);
  ASW_CHECK_ARG(radius >= 1, "lattice_nms: radius = %d, must be at least 1", radius);
  if (N == 0) return ASW_OK;
  ASW_CHECK_ARG(cells && scores && workspace, "lattice_nms: null pointer");
  ASW_CHECK_ARG(best && degree, "lattice_nms: null output pointer");
  const int splits = nms_splits(N);
  const size_t slot = align256((size_t)splits * (size_t)N * sizeof(int32_t));
  ASW_CHECK_ARG(workspace_bytes >= (int64_t)(2 * slot),
                "lattice_nms: workspace of %lld bytes is too small (asw_lattice_nms_workspace_bytes)", (long long)workspace_bytes);
  hipStream_t s = asw::as_stream(stream);
  int32_t* part_best = static_cast<int32_t*>(workspace);
  int32_t* part_degree = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + slot);
  const dim3 grid(asw::cdiv(N, kNmsTile), splits);
  if (P <= 8)
    hipLaunchKernelGGL(lattice_nms_kernel<8>, grid, dim3(kNmsTile), 0, s, cells, N, P, scores, (uint32_t)radius, part_best, part_degree);
  else if (P <= 16)
    hipLaunchKernelGGL(lattice_nms_kernel<16>, grid, dim3(kNmsTile), 0, s, cells, N, P, scores, (uint32_t)radius, part_best, part_degree);
  else
    hipLaunchKernelGGL(lattice_nms_kernel<31>, grid, dim3(kNmsTile), 0, s, cells, N, P, scores, (uint32_t)radius, part_best, part_degree);
  ASW_LAUNCH_CHECK();
  hipLaunchKernelGGL(lattice_nms_combine_kernel, dim3(asw::cdiv(N, kBlock)), dim3(kBlock), 0, s, part_best, part_degree, scores, N,
                     splits, best, degree);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}
