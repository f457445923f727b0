// torch_ops.cpp -- PyTorch-ROCm custom ops `torch.ops.asw.*` over the C ABI of libasw_hip.so.
//
// the hot path is "exposed as PyTorch-ROCm custom ops".  Every op is a thin
// adapter: TORCH_CHECK of dtype / shape / device / contiguity, output allocation with torch's
// allocator on the input's device, then ONE call of the C-ABI entry point (include/asw_hip.h)
// on that device and on torch's CURRENT HIP stream -- no hidden synchronisation, no arithmetic
// here.  A failed C-ABI call becomes a Python RuntimeError carrying asw_last_error().
//
// Replaces (reference): DataParallelSpotModel.shift_and_sep and the nn.DataParallel forward
// (sep/training/JointModel/network.py:27-104), Network.forward
// (sep/training/SpeakerLocalization/network.py:363-405), the host energy loops
// (sep/helpers/local_utils_3d.py:13-17,349-354), si_sdr pairs (sep/helpers/eval_utils.py:11-82),
// SRP_Map_WINDOW_torch (sep/Traditional_SP/SRP_Prunning.py:387-434), MUSIC_Map_WINDOW / TOPS_Map_WINDOW (:436-497), the geometry
// tables of SRP_PHAT.__init__ / Map_3D_TDoA / search_cluster (:149-180,277-344,368-381; geom_*) and the joint separation
// network's infer_sample / forward (sep/training/SpeakerSeparation/network.py:418-548).
//
// Model handles (asw_spot*, asw_sep*) are created and loaded through the C ABI
// (asw_spot_create / set_param / finalize) and passed to the ops as int64.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/asw_hip.h"

namespace {

using at::Tensor;

void check_status(int rc, const char* what) {
  TORCH_CHECK(rc == ASW_OK, "libasw_hip: ", what, " failed with status ", rc, ": ", asw_last_error());
}

void need(const Tensor& t, const char* name, at::ScalarType dtype, int64_t dim) {
  TORCH_CHECK(t.is_cuda(), name, " must be a HIP (cuda) tensor");
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype, ", got ", t.scalar_type());
  TORCH_CHECK(t.dim() == dim, name, " must have ", dim, " dimensions, got ", t.dim());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void same_device(const Tensor& a, const Tensor& b, const char* what) {
  TORCH_CHECK(a.device() == b.device(), what, " must live on the same device");
}

// Device guard + torch's current stream on the tensor's device.  PyTorch-ROCm calls its HIP
// devices "cuda", so the guard / stream accessors are the "masquerading as CUDA" ones.
struct Launch {
  c10::hip::HIPGuardMasqueradingAsCUDA guard;
  void* stream;
  explicit Launch(const Tensor& t)
      : guard(t.device()), stream(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream()) {}
};

int checked_int(int64_t v, const char* name) {
  TORCH_CHECK(v >= INT32_MIN && v <= INT32_MAX, name, " out of int32 range");
  return static_cast<int>(v);
}

// A count list as the C ABI takes it: every entry inside lo..hi, with the sum of the entries and of their squares.
struct Counts {
  std::vector<int32_t> v;
  int64_t sum = 0, squares = 0;
};

Counts checked_counts(at::IntArrayRef counts, const char* name, int64_t lo = INT32_MIN, int64_t hi = INT32_MAX) {
  Counts c;
  c.v.reserve(counts.size());
  for (size_t k = 0; k < counts.size(); ++k) {
    TORCH_CHECK(counts[k] >= lo && counts[k] <= hi, name, "[", k, "] = ", counts[k], " outside ", lo, "..", hi);
    c.v.push_back(static_cast<int32_t>(counts[k]));
    c.sum += counts[k], c.squares += counts[k] * counts[k];
  }
  return c;
}

// ---- spot network -------------------------------------------------------------------------
std::tuple<Tensor, Tensor> spot_shift_and_sep(int64_t model, const Tensor& mix, const Tensor& offsets, int64_t strict,
                                              bool circular, bool want_wave, bool want_energy, int64_t window) {
  TORCH_CHECK(model != 0, "spot_shift_and_sep: null model handle");
  need(mix, "mix", at::kFloat, 2);
  need(offsets, "offsets", at::kInt, 2);
  same_device(mix, offsets, "mix and offsets");
  const int M = checked_int(mix.size(0), "M"), T = checked_int(mix.size(1), "T"), N = checked_int(offsets.size(0), "N");
  TORCH_CHECK(offsets.size(1) == M - 1, "offsets must be [N, M-1] = [N, ", M - 1, "], got [N, ", offsets.size(1), "]");
  Tensor wave = at::empty({want_wave ? N : 0, T}, mix.options());
  Tensor energy = at::empty({want_energy ? N : 0, 2}, mix.options().dtype(at::kDouble));
  if (N == 0) return {wave, energy};
  Launch l(mix);
  check_status(asw_spot_shift_and_sep(reinterpret_cast<asw_spot*>(model), mix.data_ptr<float>(), M, T,
                                      offsets.data_ptr<int32_t>(), N, checked_int(strict, "strict"), circular ? 1 : 0,
                                      want_wave ? wave.data_ptr<float>() : nullptr,
                                      want_energy ? energy.data_ptr<double>() : nullptr, checked_int(window, "window"),
                                      l.stream),
               "asw_spot_shift_and_sep");
  return {wave, energy};
}

// candidates of several mixtures in one call: mix [K, M, T], mix_index [N] (values in [0, K): built and checked on the host
// by the caller -- reading them back here would stall the stream)
std::tuple<Tensor, Tensor> spot_shift_and_sep_multi(int64_t model, const Tensor& mix, const Tensor& offsets,
                                                    const Tensor& mix_index, int64_t strict, bool circular, bool want_wave,
                                                    bool want_energy, int64_t window) {
  TORCH_CHECK(model != 0, "spot_shift_and_sep_multi: null model handle");
  need(mix, "mix", at::kFloat, 3);
  need(offsets, "offsets", at::kInt, 2);
  need(mix_index, "mix_index", at::kInt, 1);
  same_device(mix, offsets, "mix and offsets");
  same_device(mix, mix_index, "mix and mix_index");
  const int K = checked_int(mix.size(0), "K"), M = checked_int(mix.size(1), "M"), T = checked_int(mix.size(2), "T");
  const int N = checked_int(offsets.size(0), "N");
  TORCH_CHECK(K >= 1 && offsets.size(1) == M - 1 && mix_index.size(0) == N, "offsets must be [N, M-1] and mix_index [N]");
  Tensor wave = at::empty({want_wave ? N : 0, T}, mix.options());
  Tensor energy = at::empty({want_energy ? N : 0, 2}, mix.options().dtype(at::kDouble));
  if (N == 0) return {wave, energy};
  Launch l(mix);
  check_status(asw_spot_shift_and_sep_multi(reinterpret_cast<asw_spot*>(model), mix.data_ptr<float>(), K, M, T,
                                            offsets.data_ptr<int32_t>(), mix_index.data_ptr<int32_t>(), N,
                                            checked_int(strict, "strict"), circular ? 1 : 0,
                                            want_wave ? wave.data_ptr<float>() : nullptr,
                                            want_energy ? energy.data_ptr<double>() : nullptr, checked_int(window, "window"),
                                            l.stream),
               "asw_spot_shift_and_sep_multi");
  return {wave, energy};
}

Tensor spot_forward(int64_t model, const Tensor& mix_norm, double w0, double w1) {
  TORCH_CHECK(model != 0, "spot_forward: null model handle");
  need(mix_norm, "mix", at::kFloat, 3);
  const int B = checked_int(mix_norm.size(0), "B"), M = checked_int(mix_norm.size(1), "M"), t = checked_int(mix_norm.size(2), "t");
  Tensor out = at::empty({B, t}, mix_norm.options());
  if (B == 0) return out;
  const float w[2] = {static_cast<float>(w0), static_cast<float>(w1)};
  Launch l(mix_norm);
  check_status(asw_spot_forward(reinterpret_cast<asw_spot*>(model), mix_norm.data_ptr<float>(), B, M, t, w,
                                out.data_ptr<float>(), l.stream),
               "asw_spot_forward");
  return out;
}

std::tuple<Tensor, Tensor, Tensor, Tensor> shift_norm_preproc(const Tensor& mix, const Tensor& offsets, const Tensor& w,
                                                              const Tensor& b, int64_t T_pad, bool circular) {
  need(mix, "mix", at::kFloat, 2);
  need(offsets, "offsets", at::kInt, 2);
  need(w, "w", at::kFloat, 2);
  need(b, "b", at::kFloat, 1);
  same_device(mix, offsets, "mix and offsets");
  same_device(mix, w, "mix and w");
  same_device(mix, b, "mix and b");
  const int M = checked_int(mix.size(0), "M"), T = checked_int(mix.size(1), "T"), N = checked_int(offsets.size(0), "N");
  const int C = checked_int(w.size(0), "C"), Tp = checked_int(T_pad, "T_pad");
  TORCH_CHECK(offsets.size(1) == M - 1, "offsets must be [N, M-1]");
  TORCH_CHECK(w.size(1) == M && b.size(0) == C, "w must be [C, M] and b [C]");
  TORCH_CHECK(Tp >= T, "T_pad must be >= T");
  Tensor mean = at::empty({N}, mix.options()), stdv = at::empty({N}, mix.options());
  Tensor x0 = at::empty({N, Tp, C}, mix.options());
  Tensor refn = at::zeros({N, Tp}, mix.options());
  if (N == 0) return {x0, refn, mean, stdv};
  Launch l(mix);
  check_status(asw_shift_stats(mix.data_ptr<float>(), M, T, offsets.data_ptr<int32_t>(), N, circular ? 1 : 0,
                               mean.data_ptr<float>(), stdv.data_ptr<float>(), l.stream),
               "asw_shift_stats");
  check_status(asw_shift_norm_preproc(mix.data_ptr<float>(), M, T, Tp, offsets.data_ptr<int32_t>(), N, circular ? 1 : 0,
                                      mean.data_ptr<float>(), stdv.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(), C,
                                      x0.data_ptr<float>(), refn.data_ptr<float>(), Tp, l.stream),
               "asw_shift_norm_preproc");
  return {x0, refn, mean, stdv};
}

// ---- energies / SI-SDR ----------------------------------------------------------------------
Tensor energies(const Tensor& y, int64_t window) {
  need(y, "y", at::kFloat, 2);
  const int B = checked_int(y.size(0), "B"), T = checked_int(y.size(1), "T");
  Tensor out = at::empty({B, 2}, y.options().dtype(at::kDouble));
  if (B == 0) return out;
  Launch l(y);
  check_status(asw_energies(y.data_ptr<float>(), B, T, checked_int(window, "window"), /*scratch: ignored*/ nullptr,
                            out.data_ptr<double>(), l.stream),
               "asw_energies");
  return out;
}

Tensor pair_sisdr(const Tensor& y) {
  need(y, "y", at::kFloat, 2);
  const int n = checked_int(y.size(0), "n"), T = checked_int(y.size(1), "T");
  Tensor out = at::empty({n, n}, y.options().dtype(at::kDouble));
  if (n == 0) return out;
  Launch l(y);
  check_status(asw_pair_sisdr(y.data_ptr<float>(), n, T, out.data_ptr<double>(), l.stream), "asw_pair_sisdr");
  return out;
}

Tensor segment_sisdr(const Tensor& y, const Tensor& segments, const Tensor& counts) {
  need(y, "y", at::kFloat, 2);
  need(segments, "segments", at::kInt, 3);
  need(counts, "counts", at::kInt, 1);
  same_device(y, segments, "y and segments");
  same_device(y, counts, "y and counts");
  const int n = checked_int(y.size(0), "n"), T = checked_int(y.size(1), "T"), kmax = checked_int(segments.size(1), "kmax");
  TORCH_CHECK(segments.size(0) == n && segments.size(2) == 2 && counts.size(0) == n && kmax >= 1,
              "segments must be [n, kmax, 2] and counts [n]");
  Tensor out = at::full({n, n, kmax}, std::numeric_limits<double>::quiet_NaN(), y.options().dtype(at::kDouble));
  if (n == 0) return out;
  Launch l(y);
  check_status(asw_segment_sisdr(y.data_ptr<float>(), n, T, segments.data_ptr<int32_t>(), counts.data_ptr<int32_t>(), kmax,
                                 out.data_ptr<double>(), l.stream),
               "asw_segment_sisdr");
  return out;
}

// -> segments [n, kcap, 2] int32, counts [n] int32, ms [n, 1 + T/256] float64 (empty unless want_ms): the voiced segments
// of every row (hostdsp.voiced_segments_f64), kcap = max(1, T / 1000).  The threshold and the quiet bound are formed here
// in double as the statement forms them: 10 ** (-top_db / 10) and 0.04 * 0.04.
std::tuple<Tensor, Tensor, Tensor> voiced_segments(const Tensor& y, double top_db, bool want_ms) {
  need(y, "y", at::kFloat, 2);
  const int n = checked_int(y.size(0), "n"), T = checked_int(y.size(1), "T");
  TORCH_CHECK(T >= 1, "y must hold at least one sample per row");
  TORCH_CHECK(n <= 65535, "voiced_segments takes at most 65535 waveforms, got ", n);
  const int64_t kcap = T / 1000 > 1 ? T / 1000 : 1, nfr = 1 + T / 256;
  Tensor segments = at::empty({n, kcap, 2}, y.options().dtype(at::kInt));
  Tensor counts = at::empty({n}, y.options().dtype(at::kInt));
  Tensor ms = at::empty({want_ms ? n : 0, nfr}, y.options().dtype(at::kDouble));
  if (n == 0) return {segments, counts, ms};
  const size_t ws_bytes = asw_voiced_segments_workspace_bytes(n, T);
  Tensor ws = at::empty({static_cast<int64_t>(ws_bytes / sizeof(double))}, y.options().dtype(at::kDouble));
  const double thr = std::pow(10.0, -top_db / 10.0), Q = 0.04 * 0.04;
  Launch l(y);
  check_status(asw_voiced_segments(y.data_ptr<float>(), n, T, thr, Q, segments.data_ptr<int32_t>(), static_cast<int>(kcap),
                                   counts.data_ptr<int32_t>(), want_ms ? ms.data_ptr<double>() : nullptr, ws.data_ptr(),
                                   ws_bytes, l.stream),
               "asw_voiced_segments");
  return {segments, counts, ms};
}

// -> order [N] int32, label [N] int32, gram [sum n_g^2] float64 (empty unless want_gram): the fine stage's clustering of
// every group of rows (fine_cluster.fine_clusters_f64).  bounds is a CPU tensor [G + 1] int32: the C entry point checks
// it on the host.  ratio is formed here in double as the statement forms it: 10 ** (sim_db / 10).
std::tuple<Tensor, Tensor, Tensor> fine_clusters(const Tensor& y, const Tensor& bounds, const Tensor& energies,
                                                 const Tensor& gate, const Tensor& group_gate, double min_trigger,
                                                 double sim_db, bool want_gram) {
  need(y, "y", at::kFloat, 2);
  need(energies, "energies", at::kDouble, 2);
  need(gate, "gate", at::kDouble, 1);
  need(group_gate, "group_gate", at::kDouble, 1);
  same_device(y, energies, "y and energies");
  same_device(y, gate, "y and gate");
  same_device(y, group_gate, "y and group_gate");
  TORCH_CHECK(bounds.is_cpu() && bounds.scalar_type() == at::kInt && bounds.dim() == 1 && bounds.is_contiguous() &&
                  bounds.size(0) >= 1,
              "bounds must be a contiguous CPU Int tensor [G + 1]");
  const int N = checked_int(y.size(0), "N"), T = checked_int(y.size(1), "T");
  const int G = checked_int(bounds.size(0) - 1, "G");
  TORCH_CHECK(T >= 1, "y must hold at least one sample per row");
  TORCH_CHECK(energies.size(0) == N && energies.size(1) == 2, "energies must be [N, 2]");
  TORCH_CHECK(gate.size(0) == N, "gate must be [N]");
  TORCH_CHECK(group_gate.size(0) == G, "group_gate must be [G]");
  const int32_t* b = bounds.data_ptr<int32_t>();
  const size_t ws_bytes = asw_fine_clusters_workspace_bytes(b, G);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_fine_clusters_workspace_bytes failed: ", asw_last_error());   // never 0 for valid bounds
  TORCH_CHECK(b[G] == N, "bounds must end at the number of rows ", N, ", got ", b[G]);
  int64_t elems = 0;
  for (int g = 0; g < G; ++g) elems += static_cast<int64_t>(b[g + 1] - b[g]) * (b[g + 1] - b[g]);
  Tensor order = at::empty({N}, y.options().dtype(at::kInt));
  Tensor label = at::empty({N}, y.options().dtype(at::kInt));
  Tensor gram = at::empty({want_gram ? elems : 0}, y.options().dtype(at::kDouble));
  if (N == 0 || G == 0) return {order, label, gram};
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, y.options().dtype(at::kDouble));
  const double ratio = std::pow(10.0, sim_db / 10.0);
  Launch l(y);
  check_status(asw_fine_clusters(y.data_ptr<float>(), N, T, b, G, energies.data_ptr<double>(), gate.data_ptr<double>(),
                                 group_gate.data_ptr<double>(), min_trigger, ratio, ws.data_ptr(), ws_bytes,
                                 order.data_ptr<int32_t>(), label.data_ptr<int32_t>(),
                                 want_gram ? gram.data_ptr<double>() : nullptr, l.stream),
               "asw_fine_clusters");
  return {order, label, gram};
}

// -> label [n] int32, merge [n, n] uint8 (empty [0, n] unless want_merge): the global clustering's decisions over the
// tensors pair_sisdr and segment_sisdr wrote (global_cluster.global_clusters_f64).  Nothing is read back.
std::tuple<Tensor, Tensor> global_clusters(const Tensor& full, const Tensor& seg, const Tensor& counts, const Tensor& near,
                                           double sim_db, double win_hi, double win_lo, double best_hi, double best_lo,
                                           bool want_merge) {
  need(full, "full", at::kDouble, 2);
  need(seg, "seg", at::kDouble, 3);
  need(counts, "counts", at::kInt, 1);
  need(near, "near", at::kByte, 2);
  same_device(full, seg, "full and seg");
  same_device(full, counts, "full and counts");
  same_device(full, near, "full and near");
  const int n = checked_int(full.size(0), "n"), K = checked_int(seg.size(2), "K");
  TORCH_CHECK(full.size(1) == n, "full must be [n, n]");
  TORCH_CHECK(seg.size(0) == n && seg.size(1) == n && K >= 1, "seg must be [n, n, K] with K >= 1");
  TORCH_CHECK(counts.size(0) == n, "counts must be [n]");
  TORCH_CHECK(near.size(0) == n && near.size(1) == n, "near must be [n, n]");
  TORCH_CHECK(n <= 8192, "global_clusters takes at most 8192 candidates, got ", n);
  Tensor label = at::empty({n}, full.options().dtype(at::kInt));
  Tensor merge = at::empty({want_merge ? n : 0, n}, full.options().dtype(at::kByte));
  if (n == 0) return {label, merge};
  const size_t ws_bytes = asw_global_clusters_workspace_bytes(n);
  Tensor ws = at::empty({static_cast<int64_t>(ws_bytes / 8)}, full.options().dtype(at::kDouble));
  Launch l(full);
  check_status(asw_global_clusters(full.data_ptr<double>(), seg.data_ptr<double>(), counts.data_ptr<int32_t>(),
                                   near.data_ptr<uint8_t>(), n, K, sim_db, win_hi, win_lo, best_hi, best_lo, ws.data_ptr(),
                                   ws_bytes, label.data_ptr<int32_t>(), want_merge ? merge.data_ptr<uint8_t>() : nullptr,
                                   l.stream),
               "asw_global_clusters");
  return {label, merge};
}

// -> kept [cap] int32, counts [2] int32, thr [2] float64: the coarse stage's decision over the N cubes of a lattice
// (search.coarse_select_f64).  Column 1 of `energies` is read where spot_shift_and_sep wrote it; nothing is read back.
std::tuple<Tensor, Tensor, Tensor> coarse_select(const Tensor& energies, const Tensor& dis1, const c10::optional<Tensor>& best,
                                                 double thr1, bool relative, double rel, int64_t cap) {
  need(energies, "energies", at::kDouble, 2);
  need(dis1, "dis1", at::kDouble, 1);
  same_device(energies, dis1, "energies and dis1");
  const int N = checked_int(energies.size(0), "N");
  TORCH_CHECK(energies.size(1) == 2, "energies must be [N, 2]");
  TORCH_CHECK(dis1.size(0) == N, "dis1 must be [N]");
  TORCH_CHECK(N <= (1 << 24), "coarse_select takes at most 2^24 cubes, got ", N);
  TORCH_CHECK(cap >= 1 && cap <= 64, "cap must lie in 1..64, got ", cap);
  const int32_t* best_p = nullptr;
  if (best.has_value()) {
    need(*best, "best", at::kInt, 1);
    same_device(energies, *best, "energies and best");
    TORCH_CHECK(best->size(0) == N, "best must be [N]");
    best_p = N > 0 ? best->data_ptr<int32_t>() : nullptr;
  }
  Tensor kept = at::empty({cap}, energies.options().dtype(at::kInt));
  Tensor counts = at::empty({2}, energies.options().dtype(at::kInt));
  Tensor thr = at::empty({2}, energies.options());
  const size_t ws_bytes = asw_coarse_select_workspace_bytes(N, static_cast<int>(cap));
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_coarse_select_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>(ws_bytes / 8)}, energies.options());
  Launch l(energies);
  check_status(asw_coarse_select(N > 0 ? energies.data_ptr<double>() : nullptr, N > 0 ? dis1.data_ptr<double>() : nullptr, best_p,
                                 N, thr1, relative ? 1 : 0, rel, static_cast<int>(cap), ws.data_ptr(), ws_bytes,
                                 kept.data_ptr<int32_t>(), counts.data_ptr<int32_t>(), thr.data_ptr<double>(), l.stream),
               "asw_coarse_select");
  return {kept, counts, thr};
}

Tensor center_rows_(Tensor y) {
  need(y, "y", at::kFloat, 2);
  if (y.size(0) == 0) return y;
  Launch l(y);
  check_status(asw_center_rows(y.data_ptr<float>(), checked_int(y.size(0), "B"), checked_int(y.size(1), "T"), l.stream),
               "asw_center_rows");
  return y;
}

// ---- SRP-PHAT map -------------------------------------------------------------------------------
Tensor srp_phat_map(const Tensor& mix, const Tensor& twiddle, const Tensor& pair_i, const Tensor& pair_j, const Tensor& tau,
                    const Tensor& omega, int64_t window, int64_t step, int64_t n_windows, int64_t nfft, int64_t hop,
                    double tol) {
  need(mix, "mix", at::kFloat, 2);
  need(twiddle, "twiddle", at::kFloat, 2);
  need(pair_i, "pair_i", at::kInt, 1);
  need(pair_j, "pair_j", at::kInt, 1);
  need(tau, "tau", at::kDouble, 2);
  need(omega, "omega", at::kDouble, 1);
  for (const Tensor* t : {&twiddle, &pair_i, &pair_j, &tau, &omega}) same_device(mix, *t, "all SRP-PHAT operands");
  const int M = checked_int(mix.size(0), "M"), T = checked_int(mix.size(1), "T");
  const int P = checked_int(pair_i.size(0), "P"), G = checked_int(tau.size(0), "G"), nbins = checked_int(omega.size(0), "nbins");
  const int nb_pad = checked_int(twiddle.size(0) / 2, "nb_pad"), nw = checked_int(n_windows, "n_windows");
  TORCH_CHECK(M >= 2 && M <= 32, "srp_phat_map: ", M, " microphones (2..32 supported)");
  TORCH_CHECK(T % 4 == 0, "mix length must be a multiple of 4 (pad with zeros)");
  TORCH_CHECK(nfft > 0 && hop > 0 && window >= nfft, "srp_phat_map: window ", window, " is shorter than one ", nfft,
              "-sample frame");
  TORCH_CHECK(twiddle.size(1) == nfft && twiddle.size(0) == 2 * (int64_t)nb_pad && nb_pad >= nbins, "twiddle must be [2*nb_pad, nfft]");
  TORCH_CHECK(pair_j.size(0) == P && tau.size(1) == M, "pair_j must be [P], tau [G, M]");
  Tensor out = at::zeros({G}, mix.options());
  if (nw <= 0 || G == 0) return out;
  TORCH_CHECK((nw - 1) * step + window <= T, "windows run past the end of the mixture");
  Launch l(mix);
  const int F = asw_srp_frames(checked_int(window, "window"), checked_int(nfft, "nfft"), checked_int(hop, "hop"));
  Tensor xf = at::empty({M, F, 2 * nb_pad}, mix.options());
  Tensor cc = at::empty({nw, nbins, P, 2}, mix.options());
  Tensor part = at::empty({8 * 8 * (int64_t)G}, mix.options());
  check_status(asw_srp_cross_spectra(mix.data_ptr<float>(), M, T, (int)window, (int)step, nw, (int)nfft, (int)hop, nbins, nb_pad,
                                     static_cast<float>(tol), twiddle.data_ptr<float>(), pair_i.data_ptr<int32_t>(),
                                     pair_j.data_ptr<int32_t>(), P, xf.data_ptr<float>(), cc.data_ptr<float>(), l.stream),
               "asw_srp_cross_spectra");
  check_status(asw_srp_map(cc.data_ptr<float>(), nw, nbins, P, tau.data_ptr<double>(), G, M, omega.data_ptr<double>(),
                           pair_i.data_ptr<int32_t>(), pair_j.data_ptr<int32_t>(), part.data_ptr<float>(), out.data_ptr<float>(),
                           l.stream),
               "asw_srp_map");
  return out;
}

// ---- MUSIC / TOPS pruning maps --------------------------------------------------------------------
// Shared by the ops below: covariance per (window, bin) + magnitude sums (asw_pruner_covariance).
std::tuple<Tensor, Tensor> covariance_impl(const Launch& l, const Tensor& mix, int bin0, int nbins, int64_t window, int64_t step,
                                           int nw, int64_t nfft, int64_t hop) {
  const int M = checked_int(mix.size(0), "M"), T = checked_int(mix.size(1), "T");
  TORCH_CHECK(nw > 0 && (nw - 1) * step + window <= T, "windows run past the end of the mixture");
  Tensor cov = at::empty({nw, nbins, M, M}, mix.options().dtype(at::kComplexDouble));
  Tensor mag = at::empty({nw, nbins}, mix.options().dtype(at::kDouble));
  check_status(asw_pruner_covariance(mix.data_ptr<float>(), M, T, checked_int(window, "window"), checked_int(step, "step"), nw,
                                     checked_int(nfft, "nfft"), checked_int(hop, "hop"), bin0, nbins,
                                     reinterpret_cast<double*>(cov.data_ptr()), mag.data_ptr<double>(), l.stream),
               "asw_pruner_covariance");
  return {cov, mag};
}

std::tuple<Tensor, Tensor> eigh_impl(const Launch& l, const Tensor& a) {
  const int M = checked_int(a.size(-1), "M");
  const int64_t n = a.numel() / ((int64_t)M * M);
  std::vector<int64_t> vshape(a.sizes().begin(), a.sizes().end() - 1);
  Tensor evals = at::empty(vshape, a.options().dtype(at::kDouble));
  Tensor evecs = at::empty(a.sizes(), a.options());
  if (n == 0) return {evals, evecs};
  check_status(asw_hermitian_eigh(reinterpret_cast<const double*>(a.data_ptr()), checked_int(n, "n"), M, evals.data_ptr<double>(),
                                  reinterpret_cast<double*>(evecs.data_ptr()), l.stream),
               "asw_hermitian_eigh");
  return {evals, evecs};
}

std::tuple<Tensor, Tensor> pruner_covariance(const Tensor& mix, int64_t bin0, int64_t nbins, int64_t window, int64_t step,
                                             int64_t n_windows, int64_t nfft, int64_t hop) {
  need(mix, "mix", at::kFloat, 2);
  Launch l(mix);
  return covariance_impl(l, mix, checked_int(bin0, "bin0"), checked_int(nbins, "nbins"), window, step,
                         checked_int(n_windows, "n_windows"), nfft, hop);
}

std::tuple<Tensor, Tensor> hermitian_eigh(const Tensor& a) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kComplexDouble && a.is_contiguous(), "a must be a contiguous complex128 HIP tensor");
  TORCH_CHECK(a.dim() >= 2 && a.size(-1) == a.size(-2) && a.size(-1) >= 1 && a.size(-1) <= 16, "a must be [..., M, M] with M <= 16");
  Launch l(a);
  return eigh_impl(l, a);
}

Tensor music_map(const Tensor& mix, const Tensor& tau, const Tensor& omega, int64_t bin0, int64_t window, int64_t step,
                 int64_t n_windows, int64_t nfft, int64_t hop) {
  need(mix, "mix", at::kFloat, 2);
  need(tau, "tau", at::kDouble, 2);
  need(omega, "omega", at::kDouble, 1);
  for (const Tensor* t : {&tau, &omega}) same_device(mix, *t, "all MUSIC operands");
  const int M = checked_int(mix.size(0), "M"), G = checked_int(tau.size(0), "G"), nbins = checked_int(omega.size(0), "nbins");
  const int nw = checked_int(n_windows, "n_windows");
  TORCH_CHECK(tau.size(1) == M && M >= 4 && M <= 16, "tau must be [G, M] with 4 <= M <= 16");
  Tensor out = at::zeros({G}, mix.options());
  if (G == 0) return out;
  Launch l(mix);
  auto cm = covariance_impl(l, mix, checked_int(bin0, "bin0"), nbins, window, step, nw, nfft, hop);
  auto ev = eigh_impl(l, std::get<0>(cm));
  Tensor p = at::empty({nw, nbins, G}, mix.options().dtype(at::kDouble));
  Tensor mx = at::empty({nw, nbins}, mix.options().dtype(at::kDouble));
  check_status(asw_music_map(reinterpret_cast<const double*>(std::get<1>(ev).data_ptr()), nw, nbins, M, tau.data_ptr<double>(), G,
                             omega.data_ptr<double>(), p.data_ptr<double>(), mx.data_ptr<double>(), out.data_ptr<float>(), l.stream),
               "asw_music_map");
  return out;
}

std::tuple<Tensor, Tensor> tops_map(const Tensor& mix, const Tensor& delta, int64_t bin0, int64_t nbins, double coef, int64_t window,
                                    int64_t step, int64_t n_windows, int64_t nfft, int64_t hop) {
  need(mix, "mix", at::kFloat, 2);
  need(delta, "delta", at::kDouble, 2);
  same_device(mix, delta, "mix and delta");
  const int M = checked_int(mix.size(0), "M"), G = checked_int(delta.size(0), "G"), nb = checked_int(nbins, "nbins");
  const int nw = checked_int(n_windows, "n_windows");
  TORCH_CHECK(delta.size(1) == M && M >= 4 && M <= 16, "delta must be [G, M] with 4 <= M <= 16");
  TORCH_CHECK(nb >= 2, "TOPS needs more than one frequency band");
  Tensor out = at::zeros({G}, mix.options());
  Tensor max_bin = at::zeros({nw > 0 ? nw : 0}, mix.options().dtype(at::kInt));
  if (G == 0) return {out, max_bin};
  Launch l(mix);
  auto cm = covariance_impl(l, mix, checked_int(bin0, "bin0"), nb, window, step, nw, nfft, hop);
  auto ev = eigh_impl(l, std::get<0>(cm));
  Tensor q = at::empty({nw, nb - 1, 3, M - 3, M, 2}, mix.options().dtype(at::kDouble));
  check_status(asw_tops_map(reinterpret_cast<const double*>(std::get<1>(ev).data_ptr()), std::get<1>(cm).data_ptr<double>(), nw, nb,
                            checked_int(bin0, "bin0"), M, delta.data_ptr<double>(), G, coef, q.data_ptr<double>(),
                            max_bin.data_ptr<int32_t>(), out.data_ptr<float>(), l.stream),
               "asw_tops_map");
  return {out, max_bin};
}

// ---- geometry tables built on the device (csrc/geometry_kernels.hip) ---------------------------------
// The axis arrays and the microphones are float64 device tensors; border / centre are host scalars.
void need_axes(const Tensor& a, const Tensor& b, const Tensor& c, const Tensor& mics) {
  need(a, "first axis", at::kDouble, 1);
  need(b, "second axis", at::kDouble, 1);
  need(c, "third axis", at::kDouble, 1);
  need(mics, "mics", at::kDouble, 2);
  for (const Tensor* t : {&b, &c, &mics}) same_device(a, *t, "all geometry operands");
  TORCH_CHECK(mics.size(1) == 3 && mics.size(0) >= 2 && mics.size(0) <= 32, "mics must be [M, 3] with 2 <= M <= 32");
  TORCH_CHECK(a.numel() > 0 && b.numel() > 0 && c.numel() > 0, "empty axis");
}

Tensor geom_lookup_planes(const Tensor& ys, const Tensor& xs, const Tensor& zs, const Tensor& mics, double C, double FS) {
  need_axes(ys, xs, zs, mics);
  const int ny = checked_int(ys.size(0), "ny"), nx = checked_int(xs.size(0), "nx"), nz = checked_int(zs.size(0), "nz");
  const int M = checked_int(mics.size(0), "M");
  TORCH_CHECK((int64_t)ny * nx * nz <= INT32_MAX, "lookup grid too large");
  Tensor planes = at::empty({M - 1, ny, nx, nz}, ys.options());
  Launch l(ys);
  check_status(asw_geom_lookup_planes(ys.data_ptr<double>(), ny, xs.data_ptr<double>(), nx, zs.data_ptr<double>(), nz,
                                      mics.data_ptr<double>(), M, C, FS, planes.data_ptr<double>(), l.stream),
               "asw_geom_lookup_planes");
  return planes;
}

std::tuple<Tensor, Tensor, Tensor> geom_voxel_map(const Tensor& xs, const Tensor& ys, const Tensor& zs, const Tensor& mics,
                                                  c10::ArrayRef<double> border, c10::ArrayRef<double> centre, double C, double FS,
                                                  double resolution) {
  need_axes(xs, ys, zs, mics);
  TORCH_CHECK(border.size() == 4 && centre.size() == 3, "border must hold 4 values and centre 3");
  const int Lx = checked_int(xs.size(0), "Lx"), Ly = checked_int(ys.size(0), "Ly"), Lz = checked_int(zs.size(0), "Lz");
  const int M = checked_int(mics.size(0), "M");
  const int64_t n = (int64_t)Lx * Ly * Lz;
  TORCH_CHECK(n <= (1 << 24), "SRP lattice too large");
  Tensor q = at::empty({n, M - 1}, xs.options().dtype(at::kInt));
  Tensor valid = at::empty({n}, xs.options().dtype(at::kByte));
  Tensor dis = at::empty({Lx, Ly}, xs.options());
  Launch l(xs);
  check_status(asw_geom_voxel_map(xs.data_ptr<double>(), Lx, ys.data_ptr<double>(), Ly, zs.data_ptr<double>(), Lz,
                                  mics.data_ptr<double>(), M, border.data(), centre.data(), C, FS, resolution,
                                  q.data_ptr<int32_t>(), valid.data_ptr<uint8_t>(), dis.data_ptr<double>(), l.stream),
               "asw_geom_voxel_map");
  return {q, valid, dis};
}

std::tuple<Tensor, int64_t> geom_label(const Tensor& q, const Tensor& valid, int64_t Lx, int64_t Ly, int64_t Lz) {
  need(q, "q", at::kInt, 2);
  need(valid, "valid", at::kByte, 1);
  same_device(q, valid, "q and valid");
  TORCH_CHECK(Lx > 0 && Ly > 0 && Lz > 0 && Lx * Ly * Lz == valid.size(0) && q.size(0) == valid.size(0) && valid.size(0) <= (1 << 24),
              "q must be [Lx*Ly*Lz, P] and valid [Lx*Ly*Lz]");
  TORCH_CHECK(q.size(1) >= 1 && q.size(1) <= 31, "q must hold 1..31 pairs");
  Tensor labels = at::empty({valid.size(0)}, q.options());
  Tensor adj = at::empty({valid.size(0)}, q.options());
  Tensor flag = at::empty({1}, q.options());
  int sweeps = 0;
  Launch l(q);
  check_status(asw_geom_label(q.data_ptr<int32_t>(), valid.data_ptr<uint8_t>(), checked_int(Lx, "Lx"), checked_int(Ly, "Ly"),
                              checked_int(Lz, "Lz"), checked_int(q.size(1), "P"), reinterpret_cast<uint32_t*>(adj.data_ptr<int32_t>()),
                              flag.data_ptr<int32_t>(), labels.data_ptr<int32_t>(), &sweeps, l.stream),
               "asw_geom_label");
  return {labels, (int64_t)sweeps};
}

// -> power_index [n], valid_flat [V], valid_cid [V], members [V], bounds [G+1], offsets [G,P], centres [G,3], tau [G,M], delta [G,M]
std::vector<Tensor> geom_compact(const Tensor& labels, const Tensor& q, const Tensor& xs, const Tensor& ys, const Tensor& zs,
                                 const Tensor& mics, c10::ArrayRef<double> centre, double C) {
  need_axes(xs, ys, zs, mics);
  need(labels, "labels", at::kInt, 1);
  need(q, "q", at::kInt, 2);
  same_device(xs, labels, "axes and labels");
  same_device(xs, q, "axes and q");
  TORCH_CHECK(centre.size() == 3, "centre must hold 3 values");
  const int Lx = checked_int(xs.size(0), "Lx"), Ly = checked_int(ys.size(0), "Ly"), Lz = checked_int(zs.size(0), "Lz");
  const int M = checked_int(mics.size(0), "M");
  const int64_t n = (int64_t)Lx * Ly * Lz;
  TORCH_CHECK(n <= (1 << 24) && labels.size(0) == n && q.size(0) == n && q.size(1) == M - 1,
              "labels must be [Lx*Ly*Lz] and q [Lx*Ly*Lz, M-1]");
  const int64_t ws_bytes = asw_geom_workspace_bytes((int)n);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_geom_workspace_bytes failed: ", asw_last_error());
  auto i32 = labels.options();
  Tensor ws = at::empty({ws_bytes}, i32.dtype(at::kByte));
  Tensor power_index = at::empty({n}, i32), valid_flat = at::empty({n}, i32), valid_cid = at::empty({n}, i32);
  Tensor members = at::empty({n}, i32), bounds = at::empty({n + 1}, i32), offsets = at::empty({n, M - 1}, i32);
  Tensor centres = at::empty({n, 3}, xs.options()), tau = at::empty({n, M}, xs.options()), delta = at::empty({n, M}, xs.options());
  int counts[2] = {0, 0};
  Launch l(xs);
  check_status(asw_geom_compact(labels.data_ptr<int32_t>(), q.data_ptr<int32_t>(), xs.data_ptr<double>(), Lx, ys.data_ptr<double>(), Ly,
                                zs.data_ptr<double>(), Lz, mics.data_ptr<double>(), M, centre.data(), C, ws.data_ptr(), ws_bytes,
                                power_index.data_ptr<int32_t>(), valid_flat.data_ptr<int32_t>(), valid_cid.data_ptr<int32_t>(),
                                members.data_ptr<int32_t>(), bounds.data_ptr<int32_t>(), offsets.data_ptr<int32_t>(),
                                centres.data_ptr<double>(), tau.data_ptr<double>(), delta.data_ptr<double>(), counts, l.stream),
               "asw_geom_compact");
  const int64_t G = counts[0], V = counts[1];
  // the [G, ...] tables outlive the build (tau and delta stay on the device for the maps): own storage, not a slice of [n, ...]
  return {power_index, valid_flat.narrow(0, 0, V), valid_cid.narrow(0, 0, V), members.narrow(0, 0, V), bounds.narrow(0, 0, G + 1),
          offsets.narrow(0, 0, G), centres.narrow(0, 0, G).clone(), tau.narrow(0, 0, G).clone(), delta.narrow(0, 0, G).clone()};
}

// -> cells [N,P] int32, bounds [N+1] int32, members [K] int32, centres [N,3] double: the coarse TDoA lattice of a lookup grid
// (dense_grid.coarse_lattice).  planes [P,ny,nx,nz] stays where it is: the device build hands over the tensor it made.
std::vector<Tensor> geom_lattice(const Tensor& planes, const Tensor& xs, const Tensor& ys, const Tensor& zs,
                                 c10::ArrayRef<double> border, double width) {
  need(planes, "planes", at::kDouble, 4);
  need(xs, "xs", at::kDouble, 1);
  need(ys, "ys", at::kDouble, 1);
  need(zs, "zs", at::kDouble, 1);
  for (const Tensor* t : {&xs, &ys, &zs}) same_device(planes, *t, "planes and axes");
  TORCH_CHECK(border.size() == 4, "border must hold 4 values");
  const int P = checked_int(planes.size(0), "P"), ny = checked_int(planes.size(1), "ny"), nx = checked_int(planes.size(2), "nx");
  const int nz = checked_int(planes.size(3), "nz");
  TORCH_CHECK(P >= 1 && P <= 31, "planes must hold 1..31 pairs");
  TORCH_CHECK(ys.size(0) == ny && xs.size(0) == nx && zs.size(0) == nz, "planes must be [P, len(ys), len(xs), len(zs)]");
  const int64_t n = (int64_t)ny * nx * nz;
  TORCH_CHECK(n > 0 && n <= INT32_MAX, "lookup grid empty or too large");
  const int64_t ws_bytes = asw_geom_lattice_workspace_bytes((int)n, P);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_geom_lattice_workspace_bytes failed: ", asw_last_error());
  auto i32 = planes.options().dtype(at::kInt);
  Tensor ws = at::empty({ws_bytes}, i32.dtype(at::kByte));
  Tensor cells = at::empty({n, P}, i32), bounds = at::empty({n + 1}, i32), members = at::empty({n}, i32);
  Tensor centres = at::empty({n, 3}, planes.options());
  int counts[2] = {0, 0};
  Launch l(planes);
  check_status(asw_geom_lattice(planes.data_ptr<double>(), P, ny, nx, nz, xs.data_ptr<double>(), ys.data_ptr<double>(),
                                zs.data_ptr<double>(), border.data(), width, ws.data_ptr(), ws_bytes, cells.data_ptr<int32_t>(),
                                bounds.data_ptr<int32_t>(), members.data_ptr<int32_t>(), centres.data_ptr<double>(), counts, l.stream),
               "asw_geom_lattice");
  const int64_t N = counts[0], K = counts[1];
  return {cells.narrow(0, 0, N), bounds.narrow(0, 0, N + 1), members.narrow(0, 0, K), centres.narrow(0, 0, N)};
}

// -> best [N] int32, degree [N] int32: non-maximum suppression over a lattice (dense_grid.lattice_local_maxima).  cells [N,P]
// is the table geom_lattice returned, read where it is; column 0 must be non-decreasing (the caller checks it).
std::vector<Tensor> lattice_nms(const Tensor& cells, const Tensor& scores, int64_t radius) {
  need(cells, "cells", at::kInt, 2);
  need(scores, "scores", at::kDouble, 1);
  same_device(cells, scores, "cells and scores");
  const int N = checked_int(cells.size(0), "N"), P = checked_int(cells.size(1), "P");
  TORCH_CHECK(P >= 1 && P <= 31, "cells must hold 1..31 pairs");
  TORCH_CHECK(scores.size(0) == N, "scores must be [N] = [", N, "], got [", scores.size(0), "]");
  TORCH_CHECK(radius >= 1, "radius must be at least 1");
  const int64_t ws_bytes = asw_lattice_nms_workspace_bytes(N, P);
  TORCH_CHECK(ws_bytes >= 0, "libasw_hip: asw_lattice_nms_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({ws_bytes}, cells.options().dtype(at::kByte));
  Tensor best = at::empty({N}, cells.options()), degree = at::empty({N}, cells.options());
  Launch l(cells);
  check_status(asw_lattice_nms(cells.data_ptr<int32_t>(), N, P, scores.data_ptr<double>(), checked_int(radius, "radius"),
                               ws.data_ptr(), ws_bytes, best.data_ptr<int32_t>(), degree.data_ptr<int32_t>(), l.stream),
               "asw_lattice_nms");
  return {best, degree};
}

// ---- joint separation network ---------------------------------------------------------------------
Tensor sep_infer(int64_t model, const Tensor& mix, const Tensor& offsets) {
  TORCH_CHECK(model != 0, "sep_infer: null model handle");
  need(mix, "mix", at::kFloat, 2);
  need(offsets, "offsets", at::kInt, 2);
  same_device(mix, offsets, "mix and offsets");
  const int M = checked_int(mix.size(0), "M"), T = checked_int(mix.size(1), "T"), S = checked_int(offsets.size(0), "S");
  TORCH_CHECK(offsets.size(1) == M - 1, "offsets must be [S, M-1]");
  Tensor out = at::empty({S, T}, mix.options());
  if (S == 0) return out;
  Launch l(mix);
  check_status(asw_sep_infer(reinterpret_cast<asw_sep*>(model), mix.data_ptr<float>(), M, T, offsets.data_ptr<int32_t>(), S,
                             out.data_ptr<float>(), l.stream),
               "asw_sep_infer");
  return out;
}

// infer_sample for K mixtures in one call: mix [K, M, T], offsets [N, M-1] item after item, counts[k] talkers in item k
Tensor sep_infer_batch(int64_t model, const Tensor& mix, const Tensor& offsets, at::IntArrayRef counts) {
  TORCH_CHECK(model != 0, "sep_infer_batch: null model handle");
  need(mix, "mix", at::kFloat, 3);
  need(offsets, "offsets", at::kInt, 2);
  same_device(mix, offsets, "mix and offsets");
  const int K = checked_int(mix.size(0), "K"), M = checked_int(mix.size(1), "M"), T = checked_int(mix.size(2), "T");
  const int N = checked_int(offsets.size(0), "N");
  TORCH_CHECK((int64_t)counts.size() == K, "counts must hold one entry per mixture: ", counts.size(), " for ", K);
  const Counts c = checked_counts(counts, "counts");
  TORCH_CHECK(c.sum == N && offsets.size(1) == M - 1, "offsets must be [sum(counts), M-1] = [", c.sum, ", ", M - 1, "], got [", N,
              ", ", offsets.size(1), "]");
  Tensor out = at::empty({N, T}, mix.options());
  Launch l(mix);
  check_status(asw_sep_infer_batch(reinterpret_cast<asw_sep*>(model), mix.data_ptr<float>(), K, M, T,
                                   offsets.data_ptr<int32_t>(), c.v.data(), out.data_ptr<float>(), l.stream),
               "asw_sep_infer_batch");
  return out;
}

Tensor sep_forward(int64_t model, const Tensor& mix_norm, int64_t n_speakers, int64_t n_mics, int64_t max_speakers) {
  TORCH_CHECK(model != 0, "sep_forward: null model handle");
  need(mix_norm, "mix", at::kFloat, 3);
  const int B = checked_int(mix_norm.size(0), "B"), t = checked_int(mix_norm.size(2), "t");
  const int S = checked_int(n_speakers, "S"), M = checked_int(n_mics, "M");
  TORCH_CHECK(S >= 1 && mix_norm.size(1) == (int64_t)S * M, "mix must be [B, S*M, t]");
  // the library pads the rows of `out` to the HANDLE's max_speakers: the caller's view of the model must agree,
  // or the copy would run past the tensor allocated here
  asw_sep_config cfg;
  check_status(asw_sep_get_config(reinterpret_cast<asw_sep*>(model), &cfg), "asw_sep_get_config");
  TORCH_CHECK(cfg.n_mics == M, "sep_forward: n_mics=", M, " but the model was built for ", cfg.n_mics);
  TORCH_CHECK(cfg.max_speakers == max_speakers, "sep_forward: max_speakers=", max_speakers, " but the model was built for ",
              cfg.max_speakers);
  const int64_t R = S > cfg.max_speakers ? S : cfg.max_speakers;
  Tensor out = at::empty({B, R, t}, mix_norm.options());
  if (B == 0) return out;
  Launch l(mix_norm);
  check_status(asw_sep_forward(reinterpret_cast<asw_sep*>(model), mix_norm.data_ptr<float>(), B, S, M, t, out.data_ptr<float>(),
                               l.stream),
               "asw_sep_forward");
  return out;
}

// Network.forward with a speaker count per item: mix [B, S*M, t] with S = max(counts)
Tensor sep_forward_counts(int64_t model, const Tensor& mix_norm, at::IntArrayRef counts, int64_t n_mics, int64_t max_speakers) {
  TORCH_CHECK(model != 0, "sep_forward_counts: null model handle");
  need(mix_norm, "mix", at::kFloat, 3);
  const int B = checked_int(mix_norm.size(0), "B"), t = checked_int(mix_norm.size(2), "t"), M = checked_int(n_mics, "M");
  TORCH_CHECK((int64_t)counts.size() == B && B >= 1, "counts must hold one entry per batch item");
  const Counts c = checked_counts(counts, "counts");
  const int S = std::max(0, *std::max_element(c.v.begin(), c.v.end()));
  TORCH_CHECK(S >= 1 && mix_norm.size(1) == (int64_t)S * M, "mix must be [B, max(counts)*M, t]");
  asw_sep_config cfg;
  check_status(asw_sep_get_config(reinterpret_cast<asw_sep*>(model), &cfg), "asw_sep_get_config");
  TORCH_CHECK(cfg.n_mics == M && cfg.max_speakers == max_speakers, "sep_forward_counts: n_mics / max_speakers differ from the model's");
  const int64_t R = S > cfg.max_speakers ? S : cfg.max_speakers;
  Tensor out = at::empty({B, R, t}, mix_norm.options());
  Launch l(mix_norm);
  check_status(asw_sep_forward_counts(reinterpret_cast<asw_sep*>(model), mix_norm.data_ptr<float>(), B, S, M, t, c.v.data(),
                                      out.data_ptr<float>(), l.stream),
               "asw_sep_forward_counts");
  return out;
}

// The adapter of both BSS-eval ops over asw_bss_eval_sources.  -> sdr, sir, sar float64 [R, N] (all_pairs: [R, sum S_k^2], item
// k a row-major [S_k, S_k] block of (estimate, reference) per set) and status [K] int32; without want_all sir and sar stay
// undefined, the call gets null for them and the smaller workspace of asw_bss_eval_sdr_workspace_bytes.  counts is read on
// the host; an item whose status is 1 has to be recomputed by the caller (evalkit.bss_eval_sdr_batch and
// bss_eval_sources_batch do).
std::tuple<Tensor, Tensor, Tensor, Tensor> bss_eval(const Tensor& ref, const Tensor& est, at::IntArrayRef counts, int64_t flen,
                                                    bool all_pairs, bool want_all) {
  need(ref, "ref", at::kFloat, 2);
  need(est, "est", at::kFloat, 3);
  same_device(ref, est, "ref and est");
  const int N = checked_int(ref.size(0), "N"), T = checked_int(ref.size(1), "T"), R = checked_int(est.size(0), "R");
  const int K = checked_int(static_cast<int64_t>(counts.size()), "K");
  TORCH_CHECK(R >= 1, "est must hold at least one estimate set");
  TORCH_CHECK(est.size(1) == N && est.size(2) == T, "est must be [R, N, T] = [R, ", N, ", ", T, "]");
  const Counts c = checked_counts(counts, "counts", 0, 16);
  TORCH_CHECK(c.sum == N, "counts sum to ", c.sum, ", ref has ", N, " rows");
  const int64_t ncol = all_pairs ? c.squares : N;
  const auto f64 = ref.options().dtype(at::kDouble);
  Tensor sdr = at::empty({R, ncol}, f64), sir, sar;
  if (want_all) sir = at::empty({R, ncol}, f64), sar = at::empty({R, ncol}, f64);
  Tensor status = at::empty({K}, ref.options().dtype(at::kInt));
  if (K == 0) return {sdr, sir, sar, status};
  const int f = checked_int(flen, "flen"), pairs = all_pairs ? 1 : 0;
  const size_t ws_bytes = want_all ? asw_bss_eval_sources_workspace_bytes(c.v.data(), K, R, T, f, pairs)
                                   : asw_bss_eval_sdr_workspace_bytes(c.v.data(), K, R, T, f);
  TORCH_CHECK(ws_bytes > 0 || N == 0, "libasw_hip: asw_bss_eval_", want_all ? "sources" : "sdr",
              "_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, f64);
  const bool some = N > 0;
  Launch l(ref);
  check_status(asw_bss_eval_sources(some ? ref.data_ptr<float>() : nullptr, some ? est.data_ptr<float>() : nullptr, c.v.data(), K, R,
                                    T, f, pairs, some ? sdr.data_ptr<double>() : nullptr,
                                    some && want_all ? sir.data_ptr<double>() : nullptr,
                                    some && want_all ? sar.data_ptr<double>() : nullptr, status.data_ptr<int32_t>(),
                                    some ? ws.data_ptr() : nullptr, ws_bytes, l.stream),
               "asw_bss_eval_sources");
  return {sdr, sir, sar, status};
}

// -> sdr [R, N] float64, status [K] int32: the BSS-eval SDR of every estimate set of a ragged batch against its
// references (evalkit.bss_eval_sdr per item).
std::tuple<Tensor, Tensor> bss_eval_sdr(const Tensor& ref, const Tensor& est, at::IntArrayRef counts, int64_t flen) {
  auto [sdr, sir, sar, status] = bss_eval(ref, est, counts, flen, false, false);
  return {sdr, status};
}

// -> sdr, sir, sar, status: the full BSS-eval of a ragged batch (evalkit.bss_eval_sources / bss_eval_matrices per item).
std::tuple<Tensor, Tensor, Tensor, Tensor> bss_eval_sources(const Tensor& ref, const Tensor& est, at::IntArrayRef counts,
                                                            int64_t flen, bool all_pairs) {
  return bss_eval(ref, est, counts, flen, all_pairs, true);
}

// -> out float64 [sum P_k S_k], status [K] int32: the SI-SDR of every (estimate, reference) pair of a ragged batch, item
// k a row-major [P_k, S_k] block of out (hostdsp.si_sdr per pair).  Both count lists are read on the host; an item whose
// status is 1 has to be recomputed by the caller (evalkit.cross_sisdr_batch does).
std::tuple<Tensor, Tensor> cross_sisdr(const Tensor& est, const Tensor& ref, at::IntArrayRef est_counts,
                                       at::IntArrayRef ref_counts) {
  need(est, "est", at::kFloat, 2);
  need(ref, "ref", at::kFloat, 2);
  same_device(est, ref, "est and ref");
  const int T = checked_int(est.size(1), "T");
  const int K = checked_int(static_cast<int64_t>(est_counts.size()), "K");
  TORCH_CHECK(ref.size(1) == T, "est [NE, ", T, "] and ref [NR, ", ref.size(1), "] differ in length");
  TORCH_CHECK(static_cast<int64_t>(ref_counts.size()) == K, "est_counts holds ", K, " items, ref_counts ", ref_counts.size());
  const Counts pc = checked_counts(est_counts, "est_counts", 0, 4096), sc = checked_counts(ref_counts, "ref_counts", 0, 64);
  const int64_t ne = pc.sum, nr = sc.sum;
  int64_t np = 0;
  for (int k = 0; k < K; ++k) np += static_cast<int64_t>(pc.v[k]) * sc.v[k];
  TORCH_CHECK(ne == est.size(0), "est_counts sum to ", ne, ", est has ", est.size(0), " rows");
  TORCH_CHECK(nr == ref.size(0), "ref_counts sum to ", nr, ", ref has ", ref.size(0), " rows");
  Tensor out = at::empty({np}, est.options().dtype(at::kDouble));
  Tensor status = at::empty({K}, est.options().dtype(at::kInt));
  if (K == 0) return {out, status};
  const size_t ws_bytes = asw_cross_sisdr_workspace_bytes(pc.v.data(), sc.v.data(), K, T);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_cross_sisdr_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, est.options().dtype(at::kDouble));
  Launch l(est);
  check_status(asw_cross_sisdr(ne > 0 ? est.data_ptr<float>() : nullptr, nr > 0 ? ref.data_ptr<float>() : nullptr, pc.v.data(),
                               sc.v.data(), K, T, np > 0 ? out.data_ptr<double>() : nullptr, status.data_ptr<int32_t>(),
                               ws.data_ptr(), ws_bytes, l.stream),
               "asw_cross_sisdr");
  return {out, status};
}

// ---- a recording as overlapping blocks (longform.py) ------------------------------------------------------------------
// -> [K, M, T]: block k is mix[:, starts[k] : starts[k] + T], zero past the end of the recording
Tensor frame_blocks(const Tensor& mix, at::IntArrayRef starts, int64_t T) {
  need(mix, "mix", at::kFloat, 2);
  const int M = checked_int(mix.size(0), "M"), Ttot = checked_int(mix.size(1), "Ttot"), t = checked_int(T, "T");
  const int K = checked_int(static_cast<int64_t>(starts.size()), "K");
  TORCH_CHECK(t >= 1, "frame_blocks: T=", T);
  const Counts a = checked_counts(starts, "starts");
  Tensor out = at::empty({K, M, t}, mix.options());
  if (K == 0 || M == 0) return out;
  Launch l(mix);
  check_status(asw_frame_blocks(mix.data_ptr<float>(), M, Ttot, a.v.data(), K, t, out.data_ptr<float>(), l.stream),
               "asw_frame_blocks");
  return out;
}

// -> [S, Ttot]: the normalised overlap-add of the rows; row_of is the [K, S] table, row-major (S = len(row_of) / K)
Tensor stitch_blocks(const Tensor& rows, const Tensor& taper, at::IntArrayRef starts, at::IntArrayRef row_of, int64_t Ttot) {
  need(rows, "rows", at::kFloat, 2);
  need(taper, "taper", at::kDouble, 1);
  same_device(rows, taper, "rows and taper");
  const int N = checked_int(rows.size(0), "N"), T = checked_int(rows.size(1), "T"), tt = checked_int(Ttot, "Ttot");
  const int K = checked_int(static_cast<int64_t>(starts.size()), "K");
  TORCH_CHECK(taper.size(0) == T, "taper must be [T] = [", T, "], got [", taper.size(0), "]");
  TORCH_CHECK(K >= 1 && row_of.size() % K == 0, "row_of must hold K x S entries: ", row_of.size(), " for K = ", K);
  TORCH_CHECK(tt >= 0, "stitch_blocks: Ttot=", Ttot);
  const int S = checked_int(static_cast<int64_t>(row_of.size()) / K, "S");
  const Counts a = checked_counts(starts, "starts"), r = checked_counts(row_of, "row_of");
  Tensor out = at::empty({S, tt}, rows.options());
  if (S == 0 || tt == 0) return out;
  Launch l(rows);
  check_status(asw_stitch_blocks(rows.data_ptr<float>(), N, taper.data_ptr<double>(), a.v.data(), r.v.data(), K, S, T, tt,
                                 out.data_ptr<float>(), l.stream),
               "asw_stitch_blocks");
  return out;
}

// ---- STFT, inverse STFT and the oracle mask baselines (oracle_masks.py) -------------------------------------------------
// -> complex128 [R, 1025, F], F = ceil(N / 1024) + 1 (oracle_masks.stft_f64)
Tensor stft(const Tensor& x) {
  need(x, "x", at::kFloat, 2);
  const int R = checked_int(x.size(0), "R"), N = checked_int(x.size(1), "N");
  TORCH_CHECK(R <= 65535, "stft: ", R, " rows (at most 65535)");
  TORCH_CHECK(N >= 2048 && N <= (1 << 25), "stft: N = ", N, " outside 2048..2^25");
  const int64_t F = (N + 1023) / 1024 + 1;
  Tensor z = at::empty({R, 1025, F}, x.options().dtype(at::kComplexDouble));
  if (R == 0) return z;
  Launch l(x);
  check_status(asw_stft(x.data_ptr<float>(), R, N, reinterpret_cast<double*>(z.data_ptr()), l.stream), "asw_stft");
  return z;
}

// -> float64 [R, n]: the first n samples of the inverse STFT of z [R, 1025, F] (oracle_masks.istft_f64)
Tensor istft(const Tensor& z, int64_t n) {
  need(z, "z", at::kComplexDouble, 3);
  const int R = checked_int(z.size(0), "R"), F = checked_int(z.size(2), "F"), N = checked_int(n, "n");
  TORCH_CHECK(z.size(1) == 1025, "z must be [R, 1025, F], got [R, ", z.size(1), ", F]");
  TORCH_CHECK(R <= 65535 && F >= 2 && F <= (1 << 15) + 1, "istft: R = ", R, " (at most 65535) or F = ", F, " outside 2..32769");
  TORCH_CHECK(N >= 0 && N <= (F - 1) * 1024, "istft: n = ", N, " outside 0..", (F - 1) * 1024, ", what ", F, " frames cover");
  Tensor out = at::empty({R, N}, z.options().dtype(at::kDouble));
  if (R == 0 || N == 0) return out;
  const size_t ws_bytes = asw_istft_workspace_bytes(R, F);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_istft_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, z.options().dtype(at::kDouble));
  Launch l(z);
  check_status(asw_istft(reinterpret_cast<const double*>(z.data_ptr()), R, F, N, out.data_ptr<double>(), ws.data_ptr(), ws_bytes,
                         l.stream),
               "asw_istft");
  return out;
}

// -> float64 [sum counts, T]: the ideal ratio ("irm") or ideal binary ("ibm") mask estimates of K items, item k one row
// of mix [K, T], the next counts[k] rows of ref [sum counts, T] and lengths[k] <= T samples; an output row is zero from
// lengths[k] on (oracle_masks.irm_f64 / ibm_f64 per item).  Both lists are read on the host.
Tensor oracle_masks(const Tensor& mix, const Tensor& ref, at::IntArrayRef counts, at::IntArrayRef lengths, std::string kind,
                    double alpha, double theta) {
  need(mix, "mix", at::kFloat, 2);
  need(ref, "ref", at::kFloat, 2);
  same_device(mix, ref, "mix and ref");
  const int K = checked_int(mix.size(0), "K"), T = checked_int(mix.size(1), "T");
  TORCH_CHECK(kind == "irm" || kind == "ibm", "oracle_masks: kind must be \"irm\" or \"ibm\", got \"", kind, "\"");
  TORCH_CHECK(K <= 65535, "oracle_masks: ", K, " items (at most 65535)");
  TORCH_CHECK(static_cast<int64_t>(counts.size()) == K && static_cast<int64_t>(lengths.size()) == K, "mix holds ", K,
              " items, counts ", counts.size(), ", lengths ", lengths.size());
  TORCH_CHECK(ref.size(1) == T, "mix [K, ", T, "] and ref [NR, ", ref.size(1), "] differ in length");
  TORCH_CHECK(alpha == alpha && theta == theta, "oracle_masks: alpha or theta is not a number");
  const Counts c = checked_counts(counts, "counts", 0, 64), n = checked_counts(lengths, "lengths", 2048, T);
  TORCH_CHECK(c.sum == ref.size(0), "counts sum to ", c.sum, ", ref has ", ref.size(0), " rows");
  Tensor out = at::empty({c.sum, T}, mix.options().dtype(at::kDouble));
  if (K == 0 || c.sum == 0) return out;
  const size_t ws_bytes = asw_oracle_masks_workspace_bytes(c.v.data(), n.v.data(), K);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_oracle_masks_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, mix.options().dtype(at::kDouble));
  Launch l(mix);
  check_status(asw_oracle_masks(mix.data_ptr<float>(), ref.data_ptr<float>(), c.v.data(), n.v.data(), K, T,
                                kind == "irm" ? ASW_ORACLE_IRM : ASW_ORACLE_IBM, alpha, theta, out.data_ptr<double>(), ws.data_ptr(),
                                ws_bytes, l.stream),
               "asw_oracle_masks");
  return out;
}

// ---- room simulator (roomsim.py) ----------------------------------------------------------------------------------------
void need_host_f64(const Tensor& t, const char* name, std::initializer_list<int64_t> shape) {
  TORCH_CHECK(t.is_cpu(), name, " must be a host (cpu) tensor: the library reads it before the call returns");
  TORCH_CHECK(t.scalar_type() == at::kDouble, name, " must be float64, got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.sizes() == at::IntArrayRef(shape.begin(), shape.size()), name, " has shape ", t.sizes(), ", expected ",
              at::IntArrayRef(shape.begin(), shape.size()));
}

// -> float64 [sum counts, M, length] on the current HIP device: the image-source responses of K shoebox scenes
// (roomsim.rir_f64).  rooms [K,3], absorption [K], src [sum counts,3] and mics [K,M,3] are HOST float64 tensors and the two
// lists host integers, as the library validates all of them before its one launch; the op is registered for the CPU key.
Tensor room_rir(const Tensor& rooms, const Tensor& absorption, at::IntArrayRef max_orders, const Tensor& src, const Tensor& mics,
                at::IntArrayRef counts, double fs, int64_t length) {
  const int K = checked_int(static_cast<int64_t>(counts.size()), "K");
  TORCH_CHECK(K <= 65535, "room_rir: ", K, " scenes (at most 65535)");
  TORCH_CHECK(mics.dim() == 3, "mics must be [K, M, 3], got ", mics.dim(), " dimensions");
  const int M = checked_int(mics.size(1), "M");
  TORCH_CHECK(M >= 1 && M <= 1024, "room_rir: M = ", M, " outside 1..1024");
  TORCH_CHECK(length >= 1 && length <= (1 << 25), "room_rir: length = ", length, " outside 1..2^25");
  TORCH_CHECK(static_cast<int64_t>(max_orders.size()) == K, "counts holds ", K, " scenes, max_orders ", max_orders.size());
  const Counts c = checked_counts(counts, "counts", 0, 64), n = checked_counts(max_orders, "max_orders");
  TORCH_CHECK(c.sum <= 65535, "room_rir: ", c.sum, " sources (at most 65535)");
  need_host_f64(rooms, "rooms", {K, 3});
  need_host_f64(absorption, "absorption", {K});
  need_host_f64(src, "src", {c.sum, 3});
  need_host_f64(mics, "mics", {K, M, 3});
  const auto dev = c10::Device(c10::DeviceType::CUDA, c10::hip::current_device());
  Tensor out = at::empty({c.sum, M, length}, at::TensorOptions().dtype(at::kDouble).device(dev));
  const size_t ws_bytes = asw_room_rir_workspace_bytes(K, M, static_cast<int>(c.sum));
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_room_rir_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, out.options());
  Launch l(out);
  check_status(asw_room_rir(rooms.data_ptr<double>(), absorption.data_ptr<double>(), n.v.data(), src.data_ptr<double>(),
                            mics.data_ptr<double>(), c.v.data(), K, M, fs, static_cast<int>(length), out.data_ptr<double>(),
                            ws.data_ptr(), ws_bytes, l.stream),
               "asw_room_rir");
  return out;
}

// -> (premix float64 [sum counts, M, T], mix float64 [K, M, T]): dry [sum counts, T] float32 through rir [sum counts, M,
// length] float64, and the sum over the sources of every scene in order (roomsim.convolve_f64)
std::tuple<Tensor, Tensor> room_convolve(const Tensor& dry, const Tensor& rir, at::IntArrayRef counts) {
  need(dry, "dry", at::kFloat, 2);
  need(rir, "rir", at::kDouble, 3);
  same_device(dry, rir, "dry and rir");
  const int K = checked_int(static_cast<int64_t>(counts.size()), "K"), T = checked_int(dry.size(1), "T");
  const int M = checked_int(rir.size(1), "M"), length = checked_int(rir.size(2), "length");
  TORCH_CHECK(K <= 65535, "room_convolve: ", K, " scenes (at most 65535)");
  const Counts c = checked_counts(counts, "counts", 0, 64);
  TORCH_CHECK(c.sum == dry.size(0) && c.sum == rir.size(0), "counts sum to ", c.sum, ", dry has ", dry.size(0), " rows and rir ",
              rir.size(0));
  TORCH_CHECK(M >= 1 && M <= 1024, "room_convolve: M = ", M, " outside 1..1024");
  TORCH_CHECK(T >= 1 && T <= (1 << 25) && length >= 1 && length <= (1 << 25), "room_convolve: T = ", T, " or length = ", length,
              " outside 1..2^25");
  Tensor premix = at::empty({c.sum, M, T}, rir.options());
  Tensor mix = at::empty({K, M, T}, rir.options());
  if (K == 0) return {premix, mix};
  const size_t ws_bytes = asw_room_convolve_workspace_bytes(c.v.data(), K, M, length, T);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_room_convolve_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, rir.options());
  Launch l(dry);
  check_status(asw_room_convolve(dry.data_ptr<float>(), rir.data_ptr<double>(), c.v.data(), K, M, length, T, premix.data_ptr<double>(),
                                 mix.data_ptr<double>(), ws.data_ptr(), ws_bytes, l.stream),
               "asw_room_convolve");
  return {premix, mix};
}

// ---- training batches (train_data.py) -------------------------------------------------------------------------------
// -> float64 [rows, T] on the current HIP device: power-law noise rows (train_data.colored_noise_f64).  The keys and row
// indices are host integers, so the op has no tensor argument and is registered for every backend.
Tensor colored_noise(at::IntArrayRef row_keys, at::IntArrayRef row_ids, int64_t T, double exponent, int64_t max_rows_per_pass) {
  const int rows = checked_int(static_cast<int64_t>(row_keys.size()), "rows");
  TORCH_CHECK(static_cast<int64_t>(row_ids.size()) == rows, "row_keys holds ", rows, " rows, row_ids ", row_ids.size());
  const Counts ids = checked_counts(row_ids, "row_ids", 0, INT32_MAX);
  const std::vector<int64_t> keys(row_keys.begin(), row_keys.end());
  const auto dev = c10::Device(c10::DeviceType::CUDA, c10::hip::current_device());
  Tensor out = at::empty({rows, T}, at::TensorOptions().dtype(at::kDouble).device(dev));
  const size_t ws_bytes = asw_colored_noise_workspace_bytes(rows, checked_int(T, "T"), checked_int(max_rows_per_pass, "max_rows_per_pass"));
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_colored_noise_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, out.options());
  Launch l(out);
  check_status(asw_colored_noise(keys.data(), ids.v.data(), rows, static_cast<int>(T), exponent, static_cast<int>(max_rows_per_pass),
                                 out.data_ptr<double>(), ws.data_ptr(), ws_bytes, l.stream),
               "asw_colored_noise");
  return out;
}

// -> [items, S_max * M, T] float32 (float64 when out_f64): mix [K, M, T] rolled per item and talker block and perturbed
// (train_data.train_batch_f64).  shifts is the flattened [items, S_max, M] table; pink [items, S_max * M, T] float64 or None
Tensor train_batch(const Tensor& mix, at::IntArrayRef item_mix, at::IntArrayRef shifts, int64_t S_max, at::IntArrayRef counts,
                   at::ArrayRef<double> pink_level, at::ArrayRef<double> white_level, at::IntArrayRef white_key,
                   const c10::optional<Tensor>& pink, bool out_f64) {
  need(mix, "mix", at::kFloat, 3);
  const int K = checked_int(mix.size(0), "K"), M = checked_int(mix.size(1), "M"), T = checked_int(mix.size(2), "T");
  const int items = checked_int(static_cast<int64_t>(item_mix.size()), "items"), S = checked_int(S_max, "S_max");
  TORCH_CHECK(S >= 1 && M >= 1, "train_batch: S_max = ", S, " or M = ", M, " below 1");
  TORCH_CHECK(static_cast<int64_t>(counts.size()) == items && static_cast<int64_t>(pink_level.size()) == items &&
                  static_cast<int64_t>(white_level.size()) == items && static_cast<int64_t>(white_key.size()) == items,
              "train_batch: item_mix holds ", items, " items, the other tables do not");
  TORCH_CHECK(static_cast<int64_t>(shifts.size()) == static_cast<int64_t>(items) * S * M, "train_batch: shifts holds ", shifts.size(),
              " entries, expected items * S_max * M = ", static_cast<int64_t>(items) * S * M);
  const Counts im = checked_counts(item_mix, "item_mix"), sh = checked_counts(shifts, "shifts"), cn = checked_counts(counts, "counts", 0, S);
  const std::vector<int64_t> keys(white_key.begin(), white_key.end());
  if (pink.has_value()) {
    need(*pink, "pink", at::kDouble, 3);
    same_device(mix, *pink, "mix and pink");
    TORCH_CHECK(pink->size(0) == items && pink->size(1) == static_cast<int64_t>(S) * M && pink->size(2) == T,
                "pink must be [items, S_max * M, T]");
  }
  Tensor out = at::empty({items, static_cast<int64_t>(S) * M, T}, mix.options().dtype(out_f64 ? at::kDouble : at::kFloat));
  if (items == 0) return out;
  const size_t ws_bytes = asw_train_batch_workspace_bytes(items, S, M);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_train_batch_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, mix.options().dtype(at::kDouble));
  Launch l(mix);
  check_status(asw_train_batch(mix.data_ptr<float>(), K, M, T, items, S, im.v.data(), sh.v.data(), cn.v.data(), pink_level.data(),
                               white_level.data(), keys.data(), pink.has_value() ? pink->data_ptr<double>() : nullptr, out.data_ptr(),
                               out_f64 ? 1 : 0, ws.data_ptr(), ws_bytes, l.stream),
               "asw_train_batch");
  return out;
}

// -> float64 [N, 4]: mean |e - g|, -SNR, -SI-SDR and max |g| of every row (train_data.row_losses_f64)
Tensor train_losses(const Tensor& est, const Tensor& gt) {
  need(est, "est", at::kFloat, 2);
  need(gt, "gt", at::kFloat, 2);
  same_device(est, gt, "est and gt");
  TORCH_CHECK(est.sizes() == gt.sizes(), "est and gt must have one shape");
  const int N = checked_int(est.size(0), "N"), T = checked_int(est.size(1), "T");
  Tensor out = at::empty({N, 4}, est.options().dtype(at::kDouble));
  if (N == 0) return out;
  Launch l(est);
  check_status(asw_train_losses(est.data_ptr<float>(), gt.data_ptr<float>(), N, T, out.data_ptr<double>(), l.stream), "asw_train_losses");
  return out;
}

// ---- corpus voices (voiceprep.py) ---------------------------------------------------------------------------------------
// -> [n, T_out] float32 or (out_f64) float64: the rows of the packed x float32 [x_len], resampled by up/down through the
// filter table h float64 (voiceprep.resample_filter) and windowed (voiceprep.resample_poly_f64, window_f64).  The four row
// tables are host integers, validated by the library before its launch.
Tensor voice_resample(const Tensor& x, at::IntArrayRef row_offset, at::IntArrayRef row_len, int64_t up, int64_t down, const Tensor& h,
                      at::IntArrayRef win_begin, at::IntArrayRef win_len, int64_t T_out, bool out_f64) {
  need(x, "x", at::kFloat, 1);
  need(h, "h", at::kDouble, 1);
  same_device(x, h, "x and h");
  const int n = checked_int(static_cast<int64_t>(row_len.size()), "n");
  TORCH_CHECK(n <= 65535, "voice_resample takes at most 65535 rows, got ", n);
  TORCH_CHECK(static_cast<int64_t>(row_offset.size()) == n && static_cast<int64_t>(win_begin.size()) == n &&
                  static_cast<int64_t>(win_len.size()) == n,
              "voice_resample: row_len holds ", n, " rows, the other tables do not");
  TORCH_CHECK(T_out >= 1 && T_out <= (1 << 30), "voice_resample: T_out = ", T_out, " outside 1..2^30");
  const Counts len = checked_counts(row_len, "row_len", 0, INT32_MAX), wl = checked_counts(win_len, "win_len", 0, T_out);
  const std::vector<int64_t> off(row_offset.begin(), row_offset.end()), wb(win_begin.begin(), win_begin.end());
  Tensor out = at::empty({n, T_out}, x.options().dtype(out_f64 ? at::kDouble : at::kFloat));
  const size_t ws_bytes = asw_voice_resample_workspace_bytes(n);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_voice_resample_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, x.options().dtype(at::kDouble));
  Launch l(x);
  check_status(asw_voice_resample(x.data_ptr<float>(), x.size(0), off.data(), len.v.data(), n, checked_int(up, "up"),
                                  checked_int(down, "down"), h.data_ptr<double>(), checked_int(h.size(0), "h_len"), wb.data(),
                                  wl.v.data(), static_cast<int>(T_out), out.data_ptr(), out_f64 ? 1 : 0, ws.data_ptr(), ws_bytes,
                                  l.stream),
               "asw_voice_resample");
  return out;
}

// -> (bounds [n, 2] int32, stats [n, 2] float64): begin and end of the non-silent span of every row of the packed x, the
// peak frame mean square and the variance of the span (voiceprep.trim_f64).  The threshold is formed here in double as the
// statement forms it: 10 ** (-top_db / 10).
std::tuple<Tensor, Tensor> voice_trim(const Tensor& x, at::IntArrayRef row_offset, at::IntArrayRef row_len, double top_db) {
  need(x, "x", at::kFloat, 1);
  const int n = checked_int(static_cast<int64_t>(row_len.size()), "n");
  TORCH_CHECK(n <= 65535, "voice_trim takes at most 65535 rows, got ", n);
  TORCH_CHECK(static_cast<int64_t>(row_offset.size()) == n, "voice_trim: row_len holds ", n, " rows, row_offset ", row_offset.size());
  TORCH_CHECK(top_db == top_db, "voice_trim: top_db is not a number");
  const Counts len = checked_counts(row_len, "row_len", 0, INT32_MAX);
  const std::vector<int64_t> off(row_offset.begin(), row_offset.end());
  const int max_len = n ? *std::max_element(len.v.begin(), len.v.end()) : 0;
  Tensor bounds = at::empty({n, 2}, x.options().dtype(at::kInt));
  Tensor stats = at::empty({n, 2}, x.options().dtype(at::kDouble));
  const size_t ws_bytes = asw_voice_trim_workspace_bytes(n, max_len);
  TORCH_CHECK(ws_bytes > 0, "libasw_hip: asw_voice_trim_workspace_bytes failed: ", asw_last_error());
  Tensor ws = at::empty({static_cast<int64_t>((ws_bytes + 7) / 8)}, x.options().dtype(at::kDouble));
  Launch l(x);
  check_status(asw_voice_trim(x.data_ptr<float>(), x.size(0), off.data(), len.v.data(), n, max_len, std::pow(10.0, -top_db / 10.0),
                              bounds.data_ptr<int32_t>(), stats.data_ptr<double>(), ws.data_ptr(), ws_bytes, l.stream),
               "asw_voice_trim");
  return {bounds, stats};
}

}  // namespace

TORCH_LIBRARY(asw, m) {
  m.def("spot_shift_and_sep(int model, Tensor mix, Tensor offsets, int strict, bool circular, bool want_wave, "
        "bool want_energy, int window) -> (Tensor, Tensor)");
  m.def("spot_shift_and_sep_multi(int model, Tensor mix, Tensor offsets, Tensor mix_index, int strict, bool circular, "
        "bool want_wave, bool want_energy, int window) -> (Tensor, Tensor)");
  m.def("spot_forward(int model, Tensor mix, float w0, float w1) -> Tensor");
  m.def("shift_norm_preproc(Tensor mix, Tensor offsets, Tensor w, Tensor b, int T_pad, bool circular) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("energies(Tensor y, int window) -> Tensor");
  m.def("pair_sisdr(Tensor y) -> Tensor");
  m.def("segment_sisdr(Tensor y, Tensor segments, Tensor counts) -> Tensor");
  m.def("voiced_segments(Tensor y, float top_db=18.0, bool want_ms=False) -> (Tensor, Tensor, Tensor)");
  m.def("fine_clusters(Tensor y, Tensor bounds, Tensor energies, Tensor gate, Tensor group_gate, float min_trigger, "
        "float sim_db=-4.0, bool want_gram=False) -> (Tensor, Tensor, Tensor)");
  m.def("global_clusters(Tensor full, Tensor seg, Tensor counts, Tensor near, float sim_db=-1.0, float win_hi=-2.0, "
        "float win_lo=-7.0, float best_hi=-1.0, float best_lo=-5.0, bool want_merge=False) -> (Tensor, Tensor)");
  m.def("coarse_select(Tensor energies, Tensor dis1, Tensor? best=None, float thr1=0.008, bool relative=False, "
        "float rel=0.4, int cap=30) -> (Tensor, Tensor, Tensor)");
  m.def("bss_eval_sdr(Tensor ref, Tensor est, int[] counts, int flen=512) -> (Tensor, Tensor)");
  m.def("bss_eval_sources(Tensor ref, Tensor est, int[] counts, int flen=512, bool all_pairs=False) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("cross_sisdr(Tensor est, Tensor ref, int[] est_counts, int[] ref_counts) -> (Tensor, Tensor)");
  m.def("center_rows_(Tensor(a!) y) -> Tensor(a!)");
  m.def("srp_phat_map(Tensor mix, Tensor twiddle, Tensor pair_i, Tensor pair_j, Tensor tau, Tensor omega, int window, "
        "int step, int n_windows, int nfft, int hop, float tol) -> Tensor");
  m.def("pruner_covariance(Tensor mix, int bin0, int nbins, int window, int step, int n_windows, int nfft, int hop) "
        "-> (Tensor, Tensor)");
  m.def("hermitian_eigh(Tensor a) -> (Tensor, Tensor)");
  m.def("music_map(Tensor mix, Tensor tau, Tensor omega, int bin0, int window, int step, int n_windows, int nfft, "
        "int hop) -> Tensor");
  m.def("tops_map(Tensor mix, Tensor delta, int bin0, int nbins, float coef, int window, int step, "
        "int n_windows, int nfft, int hop) -> (Tensor, Tensor)");
  m.def("geom_lookup_planes(Tensor ys, Tensor xs, Tensor zs, Tensor mics, float C, float FS) -> Tensor");
  m.def("geom_voxel_map(Tensor xs, Tensor ys, Tensor zs, Tensor mics, float[] border, float[] centre, float C, float FS, "
        "float resolution) -> (Tensor, Tensor, Tensor)");
  m.def("geom_label(Tensor q, Tensor valid, int Lx, int Ly, int Lz) -> (Tensor, int)");
  m.def("geom_compact(Tensor labels, Tensor q, Tensor xs, Tensor ys, Tensor zs, Tensor mics, float[] centre, float C) -> Tensor[]");
  m.def("geom_lattice(Tensor planes, Tensor xs, Tensor ys, Tensor zs, float[] border, float width) -> Tensor[]");
  m.def("lattice_nms(Tensor cells, Tensor scores, int radius) -> Tensor[]");
  m.def("sep_infer(int model, Tensor mix, Tensor offsets) -> Tensor");
  m.def("sep_infer_batch(int model, Tensor mix, Tensor offsets, int[] counts) -> Tensor");
  m.def("sep_forward(int model, Tensor mix, int n_speakers, int n_mics, int max_speakers) -> Tensor");
  m.def("sep_forward_counts(int model, Tensor mix, int[] counts, int n_mics, int max_speakers) -> Tensor");
  m.def("frame_blocks(Tensor mix, int[] starts, int T) -> Tensor");
  m.def("stitch_blocks(Tensor rows, Tensor taper, int[] starts, int[] row_of, int Ttot) -> Tensor");
  m.def("stft(Tensor x) -> Tensor");
  m.def("istft(Tensor z, int n) -> Tensor");
  m.def("oracle_masks(Tensor mix, Tensor ref, int[] counts, int[] lengths, str kind, float alpha=1.0, float theta=0.5) -> "
        "Tensor");
  m.def("room_rir(Tensor rooms, Tensor absorption, int[] max_orders, Tensor src, Tensor mics, int[] counts, float fs, "
        "int length) -> Tensor");
  m.def("room_convolve(Tensor dry, Tensor rir, int[] counts) -> (Tensor, Tensor)");
  m.def("colored_noise(int[] row_keys, int[] row_ids, int T, float exponent=1.0, int max_rows_per_pass=0) -> Tensor");
  m.def("train_batch(Tensor mix, int[] item_mix, int[] shifts, int S_max, int[] counts, float[] pink_level, float[] white_level, "
        "int[] white_key, Tensor? pink=None, bool out_f64=False) -> Tensor");
  m.def("train_losses(Tensor est, Tensor gt) -> Tensor");
  m.def("voice_resample(Tensor x, int[] row_offset, int[] row_len, int up, int down, Tensor h, int[] win_begin, int[] win_len, "
        "int T_out, bool out_f64=False) -> Tensor");
  m.def("voice_trim(Tensor x, int[] row_offset, int[] row_len, float top_db=18.0) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(asw, CUDA, m) {
  m.impl("spot_shift_and_sep", &spot_shift_and_sep);
  m.impl("spot_shift_and_sep_multi", &spot_shift_and_sep_multi);
  m.impl("spot_forward", &spot_forward);
  m.impl("shift_norm_preproc", &shift_norm_preproc);
  m.impl("energies", &energies);
  m.impl("pair_sisdr", &pair_sisdr);
  m.impl("segment_sisdr", &segment_sisdr);
  m.impl("voiced_segments", &voiced_segments);
  m.impl("fine_clusters", &fine_clusters);
  m.impl("global_clusters", &global_clusters);
  m.impl("coarse_select", &coarse_select);
  m.impl("bss_eval_sdr", &bss_eval_sdr);
  m.impl("bss_eval_sources", &bss_eval_sources);
  m.impl("cross_sisdr", &cross_sisdr);
  m.impl("center_rows_", &center_rows_);
  m.impl("srp_phat_map", &srp_phat_map);
  m.impl("pruner_covariance", &pruner_covariance);
  m.impl("hermitian_eigh", &hermitian_eigh);
  m.impl("music_map", &music_map);
  m.impl("tops_map", &tops_map);
  m.impl("geom_lookup_planes", &geom_lookup_planes);
  m.impl("geom_voxel_map", &geom_voxel_map);
  m.impl("geom_label", &geom_label);
  m.impl("geom_compact", &geom_compact);
  m.impl("geom_lattice", &geom_lattice);
  m.impl("lattice_nms", &lattice_nms);
  m.impl("sep_infer", &sep_infer);
  m.impl("sep_infer_batch", &sep_infer_batch);
  m.impl("sep_forward", &sep_forward);
  m.impl("sep_forward_counts", &sep_forward_counts);
  m.impl("frame_blocks", &frame_blocks);
  m.impl("stitch_blocks", &stitch_blocks);
  m.impl("stft", &stft);
  m.impl("istft", &istft);
  m.impl("oracle_masks", &oracle_masks);
  m.impl("room_convolve", &room_convolve);
  m.impl("train_batch", &train_batch);
  m.impl("train_losses", &train_losses);
  m.impl("voice_resample", &voice_resample);
  m.impl("voice_trim", &voice_trim);
}

// room_rir takes its geometry as host tensors (the library validates it on the host) and answers on the current device
TORCH_LIBRARY_IMPL(asw, CPU, m) {
  m.impl("room_rir", &room_rir);
}

// colored_noise takes host integers only and answers on the current device
TORCH_LIBRARY_IMPL(asw, CompositeExplicitAutograd, m) {
  m.impl("colored_noise", &colored_noise);
}
