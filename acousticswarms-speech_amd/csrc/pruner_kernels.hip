// pruner_kernels.hip -- MUSIC and TOPS pruning maps on the device (the two alternatives to
// SRP-PHAT behind Mic_Array(Prone_method=...), sep/Traditional_SP/SRP_Prunning.py:436-497).
//
// Both methods share four stages:
//   covariance   per (window, bin): the STFT bin (rectangular window, hop nfft/4) as a direct DFT in
//                double, then C_k = mean_frames(X X^H), full Hermitian M x M in double; the same pass
//                writes sum_m sum_frames |X| per bin (TOPS's reference bin choice,
//                TOPS_block.py:73-75).  Double, not the f32 DFT-GEMM of the SRP map: the
//                reference's own MUSIC / TOPS maps sit within 1.5e-7 / 4.2e-7 (relative) of a float64
//                restatement, and the MUSIC peaks divide by near-zero projections.
//   eigh         batched cyclic complex Jacobi in double, one wavefront per matrix with A and
//                V in LDS; eigenvalues ascending with their eigenvector columns, as
//                numpy.linalg.eigh returns them.
//   MUSIC map    P[g,k] = 1 / sum_j |e_j^H a|^2 over the M-3 noise eigenvectors e_j (equal to
//                a^H (I - Es Es^H) a but a sum of non-negative terms), a_m = exp(+j w_k tau_gm)
//                (phase range-reduced, then sincos, all in double);
//                per-bin maximum over g, bin mean, window mean (MUSIC_block.py:15-47).
//   TOPS map     per point: 1 / s_min(D), D = [F0^H diag(conj phi_k) W_k]_k, taken as
//                1/sqrt(lambda_min) of the 3 x 3 Gram sum_k B_k B_k^H (all in double);
//                the point-independent factors Q_k = conj(F0) (x) W_k are built once per window
//                and staged through LDS in tiles of bins (TOPS_block.py:62-136).
//
// Every reduction runs in a fixed order and no float atomics are used: two calls on the same
// input are bit-identical.
#include "asw_common.h"

namespace {

constexpr int NSRC = 3;                    // num_src of the reference (MUSIC_block.py:13)
constexpr int MAXM = 16;

// grid (nbins, n_windows), block 256.  One bin of one window: X[m][f] = sum_n x[m][start + f hop + n]
// exp(-2 pi j (bin0+k) n / nfft) in double (the twiddle phase is reduced exactly as an integer index into
// a one-period cosine table), kept in LDS; then cov[w][k] = (1/F) sum_f X_f X_f^H as [M][M] complex double
// and mag[w][k] = sum_m sum_f |X[m][f]|.
__global__ __launch_bounds__(256) void pruner_cov_kernel(const float* __restrict__ mix, int M, int T, int step, int nfft,
                                                         int hop, int F, int bin0, int nbins, double* __restrict__ cov,
                                                         double* __restrict__ mag) {
  extern __shared__ double sh[];           // cos table [nfft], then X [F][M][2]
  __shared__ double smag[MAXM];
  double* ctab = sh;
  double* sx = sh + nfft;
  const int k = blockIdx.x, w = blockIdx.y;
  const int bin = bin0 + k, q = nfft / 4;
  for (int i = threadIdx.x; i < nfft; i += blockDim.x) ctab[i] = cospi(2.0 * (double)i / (double)nfft);
  __syncthreads();
  for (int i = threadIdx.x; i < F * M; i += blockDim.x) {
    const int m = i / F, f = i - m * F;
    const float* x = mix + (long)m * T + (long)w * step + (long)f * hop;
    double re = 0.0, im = 0.0;
    int j = 0;                              // (bin * n) mod nfft
    for (int n = 0; n < nfft; ++n) {
      const double v = x[n];
      re += v * ctab[j];
      im -= v * ctab[j >= q ? j - q : j + nfft - q];      // sin(2 pi j / nfft) = cos(2 pi (j - nfft/4) / nfft)
      j += bin;
      if (j >= nfft) j -= nfft;
    }
    sx[2 * (f * M + m)] = re;
    sx[2 * (f * M + m) + 1] = im;
  }
  __syncthreads();
  const int t = threadIdx.x;
  const long base = (long)w * nbins + k;
  if (t < M * M) {
    const int i = t / M, jj = t - i * M;
    double sr = 0.0, si = 0.0;
    for (int f = 0; f < F; ++f) {
      const double ar = sx[2 * (f * M + i)], ai = sx[2 * (f * M + i) + 1];
      const double br = sx[2 * (f * M + jj)], bi = sx[2 * (f * M + jj) + 1];
      sr += ar * br + ai * bi;             // X_i conj(X_j)
      si += ai * br - ar * bi;
    }
    cov[(base * M * M + t) * 2] = sr / (double)F;
    cov[(base * M * M + t) * 2 + 1] = si / (double)F;
  }
  if (t < M) {
    double s = 0.0;
    for (int f = 0; f < F; ++f) s += hypot(sx[2 * (f * M + t)], sx[2 * (f * M + t) + 1]);
    smag[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += smag[m];
    mag[base] = s;
  }
}

// grid (n), block 64 (one wavefront per matrix).  a: [n][M][M] complex double (Hermitian),
// evals: [n][M] ascending, evecs: [n][M][M] with eigenvector j in column j.
__global__ __launch_bounds__(64) void jacobi_eigh_kernel(const double* __restrict__ a, int M, double* __restrict__ evals,
                                                         double* __restrict__ evecs) {
  __shared__ double A[MAXM][MAXM][2];
  __shared__ double V[MAXM][MAXM][2];
  __shared__ double red[64];
  const long b = blockIdx.x;
  const int t = threadIdx.x;
  const double* src = a + b * M * M * 2;
  for (int e = t; e < M * M; e += 64) {
    const int r = e / M, c = e - r * M;
    // the Hermitian part of the input (the lower triangle mirrors the upper one)
    const double re = 0.5 * (src[2 * (r * M + c)] + src[2 * (c * M + r)]);
    const double im = 0.5 * (src[2 * (r * M + c) + 1] - src[2 * (c * M + r) + 1]);
    A[r][c][0] = re;
    A[r][c][1] = r == c ? 0.0 : im;
    V[r][c][0] = r == c ? 1.0 : 0.0;
    V[r][c][1] = 0.0;
  }
  __syncthreads();
  // Frobenius norm (fixed-order tree over the lanes)
  double fro = 0.0;
  for (int e = t; e < M * M; e += 64) {
    const int r = e / M, c = e - r * M;
    fro += A[r][c][0] * A[r][c][0] + A[r][c][1] * A[r][c][1];
  }
  red[t] = fro;
  __syncthreads();
  for (int s = 32; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  fro = red[0];
  __syncthreads();
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0.0;
    for (int e = t; e < M * M; e += 64) {
      const int r = e / M, c = e - r * M;
      if (r != c) off += A[r][c][0] * A[r][c][0] + A[r][c][1] * A[r][c][1];
    }
    red[t] = off;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
      if (t < s) red[t] += red[t + s];
      __syncthreads();
    }
    off = red[0];
    __syncthreads();
    if (!(off > 1e-32 * fro)) break;       // also leaves on a zero matrix
    for (int p = 0; p < M - 1; ++p)
      for (int q = p + 1; q < M; ++q) {
        // every lane derives the same rotation from the same LDS words
        const double xr = A[p][q][0], xi = A[p][q][1];
        const double r = hypot(xr, xi);
        const double app = A[p][p][0], aqq = A[q][q][0];
        if (r == 0.0 || r < 1e-300) continue;
        // a_pq = r u; J = D R D^H with D = diag(1, conj u), R the real Jacobi rotation of
        // [[app, r], [r, aqq]] (Golub & Van Loan, sym.schur2)
        const double ur = xr / r, ui = xi / r;
        const double tau = (aqq - app) / (2.0 * r);
        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + tt * tt), s = tt * c;
        // columns: A <- A J, V <- V J.  J_pp = c, J_pq = s u, J_qp = -s conj(u), J_qq = c
        if (t < M) {
          const double rpr = A[t][p][0], rpi = A[t][p][1], rqr = A[t][q][0], rqi = A[t][q][1];
          // x conj(u) and x u
          const double qcr = rqr * ur + rqi * ui, qci = rqi * ur - rqr * ui;
          const double pur = rpr * ur - rpi * ui, pui = rpr * ui + rpi * ur;
          A[t][p][0] = c * rpr - s * qcr;
          A[t][p][1] = c * rpi - s * qci;
          A[t][q][0] = s * pur + c * rqr;
          A[t][q][1] = s * pui + c * rqi;
          const double vpr = V[t][p][0], vpi = V[t][p][1], vqr = V[t][q][0], vqi = V[t][q][1];
          const double vqcr = vqr * ur + vqi * ui, vqci = vqi * ur - vqr * ui;
          const double vpur = vpr * ur - vpi * ui, vpui = vpr * ui + vpi * ur;
          V[t][p][0] = c * vpr - s * vqcr;
          V[t][p][1] = c * vpi - s * vqci;
          V[t][q][0] = s * vpur + c * vqr;
          V[t][q][1] = s * vpui + c * vqi;
        }
        __syncthreads();
        // rows: A <- J^H A.  a_p' = c a_p - s u a_q, a_q' = s conj(u) a_p + c a_q
        if (t < M) {
          const double prr = A[p][t][0], pri = A[p][t][1], qrr = A[q][t][0], qri = A[q][t][1];
          const double qur = qrr * ur - qri * ui, qui = qrr * ui + qri * ur;
          const double pcr = prr * ur + pri * ui, pci = pri * ur - prr * ui;
          A[p][t][0] = c * prr - s * qur;
          A[p][t][1] = c * pri - s * qui;
          A[q][t][0] = s * pcr + c * qrr;
          A[q][t][1] = s * pci + c * qri;
        }
        __syncthreads();
        if (t == 0) {
          A[p][q][0] = A[p][q][1] = A[q][p][0] = A[q][p][1] = 0.0;
          A[p][p][1] = A[q][q][1] = 0.0;
        }
        __syncthreads();
      }
  }
  // ascending order, ties broken by index (stable); lane j places eigenpair j
  if (t < M) {
    const double lj = A[t][t][0];
    int rank = 0;
    for (int i = 0; i < M; ++i) {
      const double li = A[i][i][0];
      rank += (li < lj) || (li == lj && i < t);
    }
    evals[b * M + rank] = lj;
    double* dst = evecs + b * M * M * 2;
    for (int r = 0; r < M; ++r) {
      dst[2 * (r * M + rank)] = V[r][t][0];
      dst[2 * (r * M + rank) + 1] = V[r][t][1];
    }
  }
}

// exp(j ph) in double, the phase range-reduced to [-pi, pi] first
__device__ __forceinline__ void steer(double ph, double& cs, double& sn) {
  const double inv2pi = 0.15915494309189535, twopi = 6.283185307179586;
  sincos(ph - twopi * rint(ph * inv2pi), &sn, &cs);
}

constexpr int MUSIC_KS = 16;               // bin slices of the MUSIC spectrum kernel

// grid (ceil(G/256), MUSIC_KS, n_windows), block 256: thread = one grid point, bins of slice y.
// p[w][k][g] = 1 / sum_{j < M-3} |e_j^H a|^2, a_m = exp(+j omega_k tau_gm), all in double.
template <int M>
__global__ __launch_bounds__(256) void music_spectrum_kernel(const double* __restrict__ evecs, int nbins,
                                                             const double* __restrict__ tau, int G,
                                                             const double* __restrict__ omega, int kps,
                                                             double* __restrict__ p) {
  constexpr int NN = M - NSRC;
  extern __shared__ double2 en[];          // [kps][NN][M] noise vectors of the slice
  const int w = blockIdx.z;
  const int k0 = blockIdx.y * kps;
  const int k1 = k0 + kps < nbins ? k0 + kps : nbins;
  for (int i = threadIdx.x; i < (k1 - k0) * NN * M; i += blockDim.x) {
    const int kk = i / (NN * M), rem = i - kk * NN * M, j = rem / M, m = rem - j * M;
    const double* v = evecs + (((long)w * nbins + k0 + kk) * M * M + m * M + j) * 2;   // column j, row m
    en[i] = make_double2(v[0], v[1]);
  }
  __syncthreads();
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int gg = g < G ? g : G - 1;
  double tg[M];
#pragma unroll
  for (int m = 0; m < M; ++m) tg[m] = tau[(long)gg * M + m];
  for (int k = k0; k < k1; ++k) {
    double ar[M], ai[M];
    const double wk = omega[k];
#pragma unroll
    for (int m = 0; m < M; ++m) steer(wk * tg[m], ar[m], ai[m]);
    const double2* e = en + (k - k0) * NN * M;
    double den = 0.0;
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      double sr = 0.0, si = 0.0;            // conj(e_j) . a
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const double2 v = e[j * M + m];
        sr += v.x * ar[m] + v.y * ai[m];
        si += v.x * ai[m] - v.y * ar[m];
      }
      den += sr * sr + si * si;
    }
    if (g < G) p[((long)w * nbins + k) * G + g] = 1.0 / fmax(den, 1e-300);
  }
}

// grid (nbins, n_windows), block 256: mx[w][k] = max_g p[w][k][g]
__global__ __launch_bounds__(256) void music_binmax_kernel(const double* __restrict__ p, int nbins, int G,
                                                           double* __restrict__ mx) {
  __shared__ double red[256];
  const double* row = p + ((long)blockIdx.y * nbins + blockIdx.x) * G;
  double m = 0.0;                           // the spectrum is positive
  for (int g = threadIdx.x; g < G; g += blockDim.x) m = fmax(m, row[g]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) mx[blockIdx.y * nbins + blockIdx.x] = red[0];
}

// out[g] = (1/W) sum_w (1/nbins) sum_k p[w][k][g] / mx[w][k]
__global__ void music_finish_kernel(const double* __restrict__ p, const double* __restrict__ mx, int W, int nbins, int G,
                                    float* __restrict__ out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  double acc = 0.0;
  for (int w = 0; w < W; ++w) {
    double s = 0.0;
    for (int k = 0; k < nbins; ++k) s += p[((long)w * nbins + k) * G + g] / mx[w * nbins + k];
    acc += s / nbins;
  }
  out[g] = (float)(acc / W);
}

// grid (n_windows), block 256.  max_bin[w] = first argmax of mag[w][:nbins]; then for k < nbins-1
// q[w][k][s][n][m] = conj(F0[m][s]) W_k[m][n], F0 = signal columns (M-3..M-1) of bin max_bin,
// W_k = noise columns (0..M-4) of bin k.
__global__ __launch_bounds__(256) void tops_factor_kernel(const double* __restrict__ evecs, const double* __restrict__ mag,
                                                          int nbins, int M, double2* __restrict__ q,
                                                          int32_t* __restrict__ max_bin) {
  __shared__ int sbin;
  const int w = blockIdx.x;
  if (threadIdx.x == 0) {
    int best = 0;
    double bv = mag[(long)w * nbins];
    for (int k = 1; k < nbins; ++k)
      if (mag[(long)w * nbins + k] > bv) { bv = mag[(long)w * nbins + k]; best = k; }
    sbin = best;
    max_bin[w] = best;
  }
  __syncthreads();
  const int NN = M - NSRC, per = NSRC * NN * M, K = nbins - 1;
  const double* f0 = evecs + ((long)w * nbins + sbin) * M * M * 2;
  for (long i = threadIdx.x; i < (long)K * per; i += blockDim.x) {
    const int k = (int)(i / per), rem = (int)(i - (long)k * per);
    const int s = rem / (NN * M), r2 = rem - s * NN * M, n = r2 / M, m = r2 - n * M;
    const double* wk = evecs + ((long)w * nbins + k) * M * M * 2;
    const double fr = f0[2 * (m * M + (M - NSRC + s))], fi = f0[2 * (m * M + (M - NSRC + s)) + 1];
    const double vr = wk[2 * (m * M + n)], vi = wk[2 * (m * M + n) + 1];
    // conj(f) * v
    q[(long)w * K * per + i] = make_double2(fr * vr + fi * vi, fr * vi - fi * vr);
  }
}

// Smallest eigenvalue of a 3 x 3 Hermitian matrix (trigonometric form of the characteristic
// polynomial's roots).
__device__ double herm3_min_eig(const double d[3], const double o[3][2]) {
  // o[0] = h01, o[1] = h02, o[2] = h12
  const double p1 = o[0][0] * o[0][0] + o[0][1] * o[0][1] + o[1][0] * o[1][0] + o[1][1] * o[1][1] +
                    o[2][0] * o[2][0] + o[2][1] * o[2][1];
  const double qm = (d[0] + d[1] + d[2]) / 3.0;
  const double a0 = d[0] - qm, a1 = d[1] - qm, a2 = d[2] - qm;
  const double p2 = a0 * a0 + a1 * a1 + a2 * a2 + 2.0 * p1;
  if (p2 <= 0.0) return qm;
  const double pp = sqrt(p2 / 6.0);
  // det(H - qm I) for Hermitian H: a0 a1 a2 + 2 Re(h01 h12 conj(h02)) - a0|h12|^2 - a1|h02|^2 - a2|h01|^2
  const double h01r = o[0][0], h01i = o[0][1], h02r = o[1][0], h02i = o[1][1], h12r = o[2][0], h12i = o[2][1];
  const double tr = h01r * h12r - h01i * h12i, ti = h01r * h12i + h01i * h12r;
  const double re3 = tr * h02r + ti * h02i;
  const double det = a0 * a1 * a2 + 2.0 * re3 - a0 * (h12r * h12r + h12i * h12i) - a1 * (h02r * h02r + h02i * h02i) -
                     a2 * (h01r * h01r + h01i * h01i);
  double r = det / (2.0 * pp * pp * pp);
  r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
  const double phi = acos(r) / 3.0;
  double lam = qm + 2.0 * pp * cos(phi + 2.0943951023931957);
  // acos loses half the digits when two roots nearly coincide: polish with Newton steps on
  // det(H - lam I), evaluated from the shifted entries
  const double n01 = h01r * h01r + h01i * h01i, n02 = h02r * h02r + h02i * h02i, n12 = h12r * h12r + h12i * h12i;
  for (int it = 0; it < 2; ++it) {
    const double b0 = d[0] - lam, b1 = d[1] - lam, b2 = d[2] - lam;
    const double f = b0 * b1 * b2 + 2.0 * re3 - b0 * n12 - b1 * n02 - b2 * n01;
    const double df = -(b0 * b1 + b0 * b2 + b1 * b2) + n01 + n02 + n12;
    if (!(fabs(df) > 0.0)) break;
    const double nl = lam - f / df;
    if (!(fabs(nl - lam) < 0.5 * pp)) break;       // keep to the root the closed form picked
    lam = nl;
  }
  return lam;
}

constexpr int TOPS_LDS = 32 * 1024;

// grid (ceil(G/256)), block 256: thread = one grid point.  For each window: Gram
// H = sum_{k < nbins-1} B_k B_k^H, B_k[s][n] = sum_m q[k][s][n][m] conj(phi_k[m]),
// phi_k[m] = exp(j coef (k - f0) delta_gm); value 1/sqrt(max(lambda_min(H), tiny)); out = window mean.
template <int M>
__global__ __launch_bounds__(256) void tops_map_kernel(const double2* __restrict__ q, const int32_t* __restrict__ max_bin,
                                                       int W, int nbins, int bin0, const double* __restrict__ delta,
                                                       int G, double coef, float* __restrict__ out) {
  constexpr int NN = M - NSRC, PER = NSRC * NN * M, KT = TOPS_LDS / (PER * 16);
  __shared__ double2 sq[KT * PER];
  const int K = nbins - 1;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int gg = g < G ? g : G - 1;
  double dl[M];
#pragma unroll
  for (int m = 0; m < M; ++m) dl[m] = delta[(long)gg * M + m];
  double acc = 0.0;
  for (int w = 0; w < W; ++w) {
    const int f0 = bin0 + max_bin[w];
    const double2* qw = q + (long)w * K * PER;
    double hd[3] = {0.0, 0.0, 0.0}, ho[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (int kt = 0; kt < K; kt += KT) {
      const int nk = K - kt < KT ? K - kt : KT;
      __syncthreads();
      for (int i = threadIdx.x; i < nk * PER; i += blockDim.x) sq[i] = qw[(long)kt * PER + i];
      __syncthreads();
      for (int kk = 0; kk < nk; ++kk) {
        const double wk = coef * (double)(kt + kk - f0);
        double pr[M], pi[M];
#pragma unroll
        for (int m = 0; m < M; ++m) steer(wk * dl[m], pr[m], pi[m]);
        const double2* qk = sq + kk * PER;
#pragma unroll
        for (int n = 0; n < NN; ++n) {
          double br[NSRC], bi[NSRC];
#pragma unroll
          for (int s = 0; s < NSRC; ++s) {
            double sr = 0.0, si = 0.0;       // q * conj(phi)
#pragma unroll
            for (int m = 0; m < M; ++m) {
              const double2 v = qk[(s * NN + n) * M + m];
              sr += v.x * pr[m] + v.y * pi[m];
              si += v.y * pr[m] - v.x * pi[m];
            }
            br[s] = sr;
            bi[s] = si;
          }
#pragma unroll
          for (int s = 0; s < NSRC; ++s) hd[s] += br[s] * br[s] + bi[s] * bi[s];
          // H[s][t] += b_s conj(b_t) for (0,1), (0,2), (1,2)
          ho[0][0] += br[0] * br[1] + bi[0] * bi[1];
          ho[0][1] += bi[0] * br[1] - br[0] * bi[1];
          ho[1][0] += br[0] * br[2] + bi[0] * bi[2];
          ho[1][1] += bi[0] * br[2] - br[0] * bi[2];
          ho[2][0] += br[1] * br[2] + bi[1] * bi[2];
          ho[2][1] += bi[1] * br[2] - br[1] * bi[2];
        }
      }
    }
    const double lmin = herm3_min_eig(hd, ho);
    acc += 1.0 / sqrt(fmax(lmin, 1e-300));
  }
  if (g < G) out[g] = (float)(acc / W);
}

}  // namespace

extern "C" int asw_pruner_covariance(const float* mix, int M, int T, int window, int step, int n_windows, int nfft,
                                     int hop, int bin0, int nbins, double* cov, double* magsum, void* stream) {
  ASW_CHECK_ARG(mix && cov && magsum, "pruner_covariance: null pointer");
  ASW_CHECK_ARG(M >= 4 && M <= MAXM && n_windows > 0 && nbins > 0 && bin0 >= 0 && nfft >= 4 && nfft % 4 == 0 &&
                    window >= nfft && hop > 0 && step > 0 && T > 0,
                "pruner_covariance: bad shape (4 <= M <= 16, nfft a multiple of 4, window >= nfft)");
  ASW_CHECK_ARG((long)(n_windows - 1) * step + window <= T, "pruner_covariance: windows run past the signal");
  const int F = asw_srp_frames(window, nfft, hop);
  const size_t smem = ((size_t)nfft + (size_t)F * M * 2) * sizeof(double);
  ASW_CHECK_ARG(smem <= 64 * 1024, "pruner_covariance: nfft %d + %d frames x %d mics exceed the LDS tile", nfft, F, M);
  hipStream_t s = asw::as_stream(stream);
  asw::ProfScope prof(s, "pruner_covariance", 2.0 * 2.0 * (double)M * F * nfft * nbins * n_windows,
                      (double)M * T * 4 + (double)n_windows * nbins * M * M * 16);
  hipLaunchKernelGGL(pruner_cov_kernel, dim3(nbins, n_windows), dim3(256), smem, s, mix, M, T, step, nfft, hop, F, bin0,
                     nbins, cov, magsum);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" int asw_hermitian_eigh(const double* a, int n, int M, double* evals, double* evecs, void* stream) {
  ASW_CHECK_ARG(a && evals && evecs, "hermitian_eigh: null pointer");
  ASW_CHECK_ARG(n > 0 && M >= 1 && M <= MAXM, "hermitian_eigh: bad shape (n > 0, 1 <= M <= 16)");
  hipLaunchKernelGGL(jacobi_eigh_kernel, dim3(n), dim3(64), 0, asw::as_stream(stream), a, M, evals, evecs);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

namespace {
template <int M>
int launch_music(const double* evecs, int W, int nbins, const double* tau, int G, const double* omega, double* p,
                 hipStream_t s) {
  const int kps = asw::cdiv(nbins, MUSIC_KS);
  const size_t smem = (size_t)kps * (M - NSRC) * M * sizeof(double2);
  hipLaunchKernelGGL(music_spectrum_kernel<M>, dim3(asw::cdiv(G, 256), MUSIC_KS, W), dim3(256), smem, s, evecs, nbins,
                     tau, G, omega, kps, p);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

template <int M>
int launch_tops(const double2* q, const int32_t* max_bin, int W, int nbins, int bin0, const double* delta, int G,
                double coef, float* out, hipStream_t s) {
  hipLaunchKernelGGL(tops_map_kernel<M>, dim3(asw::cdiv(G, 256)), dim3(256), 0, s, q, max_bin, W, nbins, bin0, delta,
                     G, coef, out);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

#define ASW_PRUNER_DISPATCH(fn, M, ...)                                                                  \
  switch (M) {                                                                                           \
    case 4: return fn<4>(__VA_ARGS__);   case 5: return fn<5>(__VA_ARGS__);   case 6: return fn<6>(__VA_ARGS__);   \
    case 7: return fn<7>(__VA_ARGS__);   case 8: return fn<8>(__VA_ARGS__);   case 9: return fn<9>(__VA_ARGS__);   \
    case 10: return fn<10>(__VA_ARGS__); case 11: return fn<11>(__VA_ARGS__); case 12: return fn<12>(__VA_ARGS__); \
    case 13: return fn<13>(__VA_ARGS__); case 14: return fn<14>(__VA_ARGS__); case 15: return fn<15>(__VA_ARGS__); \
    case 16: return fn<16>(__VA_ARGS__);                                                                 \
    default: return ::asw::set_error(ASW_ERR_ARG, "pruner: M = %d outside 4..16", M);                    \
  }
}  // namespace

extern "C" int asw_music_map(const double* evecs, int n_windows, int nbins, int M, const double* tau, int G,
                             const double* omega, double* p_scratch, double* max_scratch, float* out, void* stream) {
  ASW_CHECK_ARG(evecs && tau && omega && p_scratch && max_scratch && out, "music_map: null pointer");
  ASW_CHECK_ARG(n_windows > 0 && nbins > 0 && G > 0 && M >= 4 && M <= MAXM, "music_map: bad shape (4 <= M <= 16)");
  hipStream_t s = asw::as_stream(stream);
  asw::ProfScope prof(s, "music_map", 8.0 * (double)G * nbins * M * (M - NSRC) * n_windows,
                      (double)n_windows * nbins * G * 8 * 3 + (double)G * M * 8);
  int rc = [&]() -> int { ASW_PRUNER_DISPATCH(launch_music, M, evecs, n_windows, nbins, tau, G, omega, p_scratch, s) }();
  if (rc) return rc;
  hipLaunchKernelGGL(music_binmax_kernel, dim3(nbins, n_windows), dim3(256), 0, s, p_scratch, nbins, G, max_scratch);
  ASW_LAUNCH_CHECK();
  hipLaunchKernelGGL(music_finish_kernel, dim3(asw::cdiv(G, 256)), dim3(256), 0, s, p_scratch, max_scratch, n_windows,
                     nbins, G, out);
  ASW_LAUNCH_CHECK();
  return ASW_OK;
}

extern "C" int asw_tops_map(const double* evecs, const double* magsum, int n_windows, int nbins, int bin0, int M,
                            const double* delta, int G, double coef, double* q_scratch, int32_t* max_bin, float* out,
                            void* stream) {
  ASW_CHECK_ARG(evecs && magsum && delta && q_scratch && max_bin && out, "tops_map: null pointer");
  ASW_CHECK_ARG(n_windows > 0 && nbins >= 2 && G > 0 && M >= 4 && M <= MAXM && bin0 >= 0,
                "tops_map: bad shape (4 <= M <= 16, at least 2 bins)");
  hipStream_t s = asw::as_stream(stream);
  asw::ProfScope prof(s, "tops_map", 8.0 * (double)G * (nbins - 1) * NSRC * (M - NSRC) * (M + 2) * n_windows,
                      (double)G * M * 8 + (double)G * 4);
  hipLaunchKernelGGL(tops_factor_kernel, dim3(n_windows), dim3(256), 0, s, evecs, magsum, nbins, M,
                     reinterpret_cast<double2*>(q_scratch), max_bin);
  ASW_LAUNCH_CHECK();
  ASW_PRUNER_DISPATCH(launch_tops, M, reinterpret_cast<const double2*>(q_scratch), max_bin, n_windows, nbins, bin0,
                      delta, G, coef, out, s)
}
