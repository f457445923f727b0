// fft1024.h -- the float64 1024-point complex transform in LDS and the split / merge steps that make it the 2048-point
// real transform (1025 one-sided bins), shared by stft_kernels.hip (STFT, inverse STFT, oracle masks) and
// room_kernels.hip (overlap-save convolution).  A workgroup of 256 threads owns one frame: the 2048 real samples are
// read as 1024 complex values z[m] = x[2m] + i x[2m+1], transformed by a radix-2 Stockham FFT that ping-pongs between
// two LDS buffers (self-sorting: no bit reversal), and split into the 1025 bins; the inverse runs the same three steps
// backwards.  Real and imaginary parts live in separate arrays, so that consecutive lanes read consecutive 8-byte
// words.  No cross-lane operations, no atomics.
#pragma once
#include <cmath>

namespace asw {
namespace fft {

constexpr int NFFT = 2048, HOP = 1024, NB = 1025, NH = 1024;   // NH: the complex transform's length
constexpr int THREADS = 256;

// the twiddle table, float64, built on the host: tw[t] = exp(-2 pi i t / 2048) for t < 1024 as (cos, -sin) pairs
inline void fill_twiddles(double* tw) {
  const double pi = 3.14159265358979323846;
  for (int t = 0; t < NH; ++t) {
    tw[2 * t] = std::cos(2.0 * pi * t / NFFT);
    tw[2 * t + 1] = -std::sin(2.0 * pi * t / NFFT);
  }
}

#ifdef __HIPCC__
struct Lds {
  double re[2][NH], im[2][NH];
};

// The 1024-point transform of (re[0], im[0]) in place: ten radix-2 Stockham passes, buffer 0 -> 1 -> 0 ...; INV takes the
// conjugate twiddles (no scaling).  Enters and leaves through a barrier.
template <bool INV>
__device__ __forceinline__ void fft1024(Lds& L, const double* __restrict__ tw, int tid) {
  int src = 0;
#pragma unroll 1
  for (int ns = 1; ns < NH; ns <<= 1) {
    __syncthreads();
    const int step = NH / ns;
    for (int j = tid; j < NH / 2; j += THREADS) {
      const int k = j & (ns - 1);
      const double c = tw[2 * (k * step)], s0 = tw[2 * (k * step) + 1];
      const double s = INV ? -s0 : s0;
      const double ar = L.re[src][j], ai = L.im[src][j], xr = L.re[src][j + NH / 2], xi = L.im[src][j + NH / 2];
      const double br = xr * c - xi * s, bi = xr * s + xi * c;
      const int j0 = ((j - k) << 1) + k;
      L.re[src ^ 1][j0] = ar + br, L.im[src ^ 1][j0] = ai + bi;
      L.re[src ^ 1][j0 + ns] = ar - br, L.im[src ^ 1][j0 + ns] = ai - bi;
    }
    src ^= 1;
  }
  __syncthreads();
}

struct Cx { double r, i; };

// The one-sided bins k and 1024 - k (0 < k <= 512) of the real frame from the half-length transform Z in buffer 0:
// X[k] = E + W^k O, X[1024-k] = conj(E - W^k O) with E, O the transforms of the even and odd samples, divided by wsum
// (the STFT's sum(w); 1 for a plain transform)
__device__ __forceinline__ void split_pair(const Lds& L, const double* __restrict__ tw, int k, double wsum, Cx& xk, Cx& xm) {
  const int km = NH - k;
  const double ar = L.re[0][k], ai = L.im[0][k], br = L.re[0][km], bi = L.im[0][km];
  const double er = 0.5 * (ar + br), ei = 0.5 * (ai - bi), orr = 0.5 * (ai + bi), oi = -0.5 * (ar - br);
  const double c = tw[2 * k], s = tw[2 * k + 1];
  const double tr = orr * c - oi * s, ti = orr * s + oi * c;
  xk = Cx{(er + tr) / wsum, (ei + ti) / wsum};
  xm = Cx{(er - tr) / wsum, -(ei - ti) / wsum};
}
// bins 0 and 1024: both real
__device__ __forceinline__ void split_ends(const Lds& L, double wsum, Cx& x0, Cx& xn) {
  const double ar = L.re[0][0], ai = L.im[0][0];
  x0 = Cx{(ar + ai) / wsum, 0.0};
  xn = Cx{(ar - ai) / wsum, 0.0};
}

// The reverse: Z'[k] = E + i O and Z'[1024-k] = conj(E) + i conj(O) from the bins Y[k], Y[1024-k], written to buffer 0
// with the 1/1024 of the inverse transform folded in
__device__ __forceinline__ void merge_pair(Lds& L, const double* __restrict__ tw, int k, Cx yk, Cx ym) {
  const int km = NH - k;
  const double er = 0.5 * (yk.r + ym.r), ei = 0.5 * (yk.i - ym.i), tr = 0.5 * (yk.r - ym.r), ti = 0.5 * (yk.i + ym.i);
  const double c = tw[2 * k], s = -tw[2 * k + 1];                       // W^-k
  const double orr = tr * c - ti * s, oi = tr * s + ti * c;
  const double sc = 1.0 / NH;
  L.re[0][k] = (er - oi) * sc, L.im[0][k] = (ei + orr) * sc;
  L.re[0][km] = (er + oi) * sc, L.im[0][km] = (orr - ei) * sc;
}
__device__ __forceinline__ void merge_ends(Lds& L, double y0, double yn) {        // the imaginary parts do not count
  L.re[0][0] = 0.5 * (y0 + yn) * (1.0 / NH), L.im[0][0] = 0.5 * (y0 - yn) * (1.0 / NH);
}
#endif  // __HIPCC__

}  // namespace fft
}  // namespace asw
