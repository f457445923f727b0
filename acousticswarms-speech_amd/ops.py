"""Thin tensor-level wrappers over the individual C-ABI kernels (include/asw_hip.h).

Used by the parity tests (each kernel against the oracle) and by the host code of the
SRP-PHAT and clustering stages.  Tensors are torch CUDA tensors used purely as device
buffers; every function launches on torch's current stream.
"""
from ctypes import byref

import torch

from .native import ConvGemmArgs, MaskPathArgs, ResStackArgs, check, current_stream, lib, ptr


def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "need contiguous float32 CUDA tensor"
    return t


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """torch Conv1d weight [N, Cin, K] -> Wt [N, K*Cin] (k-major, channel fastest)."""
    N, Cin, K = w.shape
    return w.permute(0, 2, 1).reshape(N, K * Cin).contiguous()


def convgemm(A, Wt, M_out, N, Cin, taps=1, stride=1, dil=1, pad=0, bias=None, relu=False, resid=None, mul=None,
             ln=None, stats_chan_mod=0, A2=None, B=None, a_row_stride=None, a_batch_stride=None, a_len=None,
             out=None, ln_eps=1e-5, precision="f32", use_fragments=True, glu=None, glu_out=None):
    """out[b][r][n] per include/asw_hip.h:asw_convgemm_f32.  Returns (out, stats|None)."""
    _f32(A); _f32(Wt)
    if B is None:
        B = A.shape[0]
    a_row_stride = Cin if a_row_stride is None else a_row_stride
    if a_batch_stride is None:
        a_batch_stride = A[0].numel()
    if a_len is None:
        a_len = a_batch_stride
    if out is None:
        out = torch.empty((B, M_out, N), dtype=torch.float32, device=A.device)
    stats = None
    if stats_chan_mod:
        tiles = lib().asw_convgemm_stats_tiles(M_out, N)
        stats = torch.zeros((B, tiles, 4), dtype=torch.float32, device=A.device)
    a = ConvGemmArgs()
    a.A, a.A2, a.Wt = A.data_ptr(), (A2.data_ptr() if A2 is not None else None), Wt.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.resid = resid.data_ptr() if resid is not None else None
    a.mul = mul.data_ptr() if mul is not None else None
    a.ln_gamma = ln[0].data_ptr() if ln is not None else None
    a.ln_beta = ln[1].data_ptr() if ln is not None else None
    a.out = out.data_ptr()
    a.stats = stats.data_ptr() if stats is not None else None
    a.B, a.M_out, a.N, a.Cin, a.taps, a.stride, a.dil, a.pad = B, M_out, N, Cin, taps, stride, dil, pad
    a.a_row_stride, a.a_batch_stride, a.a_len = a_row_stride, a_batch_stride, a_len
    a.chan_mod, a.relu, a.ln_eps = stats_chan_mod, int(relu), ln_eps
    if glu is not None:                      # (raw [B][M_out][2N], mr [B][4], gamma [2N], beta [2N]): GroupNorm + GLU on load
        a.glu_raw, a.glu_mr, a.glu_gamma, a.glu_beta = (_f32(t).data_ptr() for t in glu)
        if glu_out is not None:
            a.glu_out = _f32(glu_out).data_ptr()
    keep = None
    if precision in ("f16x3", "f16"):
        hi, lo, shift = split_weights_f16(Wt)
        keep = (hi, lo)
        a.precision, a.w_shift, a.Wt_hi, a.Wt_lo = (1 if precision == "f16x3" else 2), shift, hi.data_ptr(), lo.data_ptr()
        if use_fragments and N % 32 == 0 and (taps * Cin) % 16 == 0:
            fh, fl, sh2 = pack_fragments_f16(Wt, N, taps * Cin)
            assert sh2 == shift
            keep = keep + (fh, fl)
            a.Wf_hi, a.Wf_lo = fh.data_ptr(), fl.data_ptr()
    check(lib().asw_convgemm_f32(byref(a), current_stream()))
    torch.cuda.current_stream().synchronize() if keep is not None else None
    return out, stats


def _resstack_args(B, T, layers, taps, precision, eps, x=None, glu=None, glu_out=None, k0=None):
    """The ResStackArgs of a launch, without its outputs, and the tensors it points into (to be kept alive until the
    launch has run).  layers: [(Wt [64][taps*64], bias, gamma, beta, dil), ...]; k0: the K of layer 0 where it is not
    taps * 64 (the source-fed form's composed weight)."""
    a = ResStackArgs()
    a.x = _f32(x).data_ptr() if x is not None else None
    a.B, a.T, a.C, a.taps, a.n_layers = B, T, 64, taps, len(layers)
    a.precision, a.ln_eps = (1 if precision == "f16x3" else 2), eps
    keep = []
    for i, (Wt, bias, gamma, beta, dil) in enumerate(layers):
        fh, fl, sh = pack_fragments_f16(_f32(Wt), 64, k0 if (i == 0 and k0) else taps * 64)
        keep.append((fh, fl))
        d = a.layer[i]
        d.Wf_hi, d.Wf_lo, d.w_shift, d.dil = fh.data_ptr(), fl.data_ptr(), sh, dil
        d.bias, d.ln_gamma, d.ln_beta = _f32(bias).data_ptr(), _f32(gamma).data_ptr(), _f32(beta).data_ptr()
    if glu is not None:
        a.glu_raw, a.glu_mr, a.glu_gamma, a.glu_beta = (_f32(t).data_ptr() for t in glu)
        if glu_out is not None:
            a.glu_out = _f32(glu_out).data_ptr()
    return a, keep


def _resstack_launch(a):
    check(lib().asw_resstack64_f16x3(byref(a), current_stream()))
    torch.cuda.current_stream().synchronize()


def resstack(x, layers, taps=7, precision="f16x3", eps=1e-5, glu=None, out=None, glu_out=None, runs_per_item=0):
    """A stack of 1..3 64-channel residual layers in one launch (include/asw_hip.h:asw_resstack64_f16x3).
    layers: [(Wt [64][taps*64], bias, gamma, beta, dil), ...]; x [B][T][64] or None with glu = (raw, mr, gamma, beta).
    runs_per_item: asw_resstack_args.runs_per_item (the fused pair's carried-halo form; < 0 switches it off)."""
    src = x if glu is None else glu[0]
    B, T = src.shape[0], src.shape[1]
    if out is None:
        out = torch.empty((B, T, 64), dtype=torch.float32, device=src.device)
    a, keep = _resstack_args(B, T, layers, taps, precision, eps, x=x, glu=glu, glu_out=glu_out)
    a.out = out.data_ptr()
    a.runs_per_item = runs_per_item
    _resstack_launch(a)
    return out


def resstack_up(x, layers, up_wt, up_bias, skip, taps=7, eps=1e-5, glu=None):
    """The stack with the next decoder block's 64 -> 64 channel stride-2 transposed convolution applied by its last
    layer (include/asw_hip.h:asw_resstack_args.up_hi).  up_wt [256][64] (pack_conv_transpose layout), up_bias [256],
    skip [B][T][64].  Returns (raw [B][T][256], partial sums [B][tiles][4]); the stack's own output is not written."""
    import ctypes
    src = x if glu is None else glu[0]
    B, T = src.shape[0], src.shape[1]
    dev = src.device
    a, keep = _resstack_args(B, T, layers, taps, "f16x3", eps, x=x, glu=glu)
    dils = (ctypes.c_int32 * 3)(*([l[4] for l in layers] + [1] * (3 - len(layers))))
    tiles = lib().asw_resstack_tiles(T, taps, len(layers), dils, int(glu is not None))
    check(min(tiles, 0))
    uh, ul, ush = pack_fragments_f16(up_wt, 256, 64, up_feed=True)
    raw = torch.full((B, T, 256), float("nan"), dtype=torch.float32, device=dev)
    stats = torch.full((B, tiles, 4), float("nan"), dtype=torch.float32, device=dev)
    a.up_hi, a.up_lo, a.up_shift = uh.data_ptr(), ul.data_ptr(), ush
    a.up_bias, a.up_skip, a.up_out, a.up_stats = _f32(up_bias).data_ptr(), _f32(skip).data_ptr(), raw.data_ptr(), stats.data_ptr()
    _resstack_launch(a)
    return raw, stats


def resstack_src(src_hi, src_lo, pre_w, pre_b, layers, taps=7, eps=1e-5, out=None, runs_per_item=0):
    """The fused pair with its first layer fed by the 8-channel source of the 1x1 convolution (pre_w [64][M], pre_b [64])
    in front of it (include/asw_hip.h:asw_resstack_args.src_hi).  src_hi / src_lo: the planes of shift_norm_src;
    layers: [(conv weight [64][64][taps] torch layout, bias, gamma, beta, dil)] * 2."""
    import ctypes
    import numpy as np
    B, T = src_hi.shape[0], src_hi.shape[1]
    dev = src_hi.device
    if out is None:
        out = torch.empty((B, T, 64), dtype=torch.float32, device=dev)
    M = pre_w.shape[1]
    wc = np.ascontiguousarray(layers[0][0].detach().cpu().numpy(), dtype=np.float32)
    wp = np.ascontiguousarray(pre_w.detach().cpu().numpy(), dtype=np.float32).reshape(64, M)
    bp = np.ascontiguousarray(pre_b.detach().cpu().numpy(), dtype=np.float32)
    comp, pre16 = np.empty((64, 64), dtype=np.float32), np.empty((64, 16), dtype=np.float32)
    check(lib().asw_compose_source_weights(ctypes.c_void_p(wc.ctypes.data), ctypes.c_void_p(wp.ctypes.data),
                                           ctypes.c_void_p(bp.ctypes.data), M, taps, ctypes.c_void_p(comp.ctypes.data),
                                           ctypes.c_void_p(pre16.ctypes.data)))
    # layer 0 runs on the composed weight; the later layers on their own, k-major
    dev_layers = [(torch.from_numpy(comp).to(dev) if i == 0 else pack_conv_weight(l[0]).to(dev),) + tuple(l[1:])
                  for i, l in enumerate(layers)]
    a, keep = _resstack_args(B, T, dev_layers, taps, "f16x3", eps, k0=64)
    a.out = out.data_ptr()
    ph, pl, psh = pack_fragments_f16(torch.from_numpy(pre16).to(dev), 64, 16)
    a.src_hi, a.src_lo, a.pre_hi, a.pre_lo, a.pre_shift = src_hi.data_ptr(), src_lo.data_ptr(), ph.data_ptr(), pl.data_ptr(), psh
    a.runs_per_item = runs_per_item
    _resstack_launch(a)
    return out


def pack_fragments_f16(Wt, N, K, up_feed=False):
    """fp32 device Wt[N][K] -> fragment-major (hi, lo) device tensors + shift (asw_pack_fragments_f16; up_feed: with
    the K order of a residual stack's UpFeed, asw_pack_up_feed_f16)."""
    import ctypes
    import numpy as np
    w = np.ascontiguousarray(Wt.detach().cpu().numpy(), dtype=np.float32).reshape(N, K)
    hi = np.empty(w.size, dtype=np.uint16)
    lo = np.empty(w.size, dtype=np.uint16)
    sh = ctypes.c_int32()
    pack = lib().asw_pack_up_feed_f16 if up_feed else lib().asw_pack_fragments_f16
    check(pack(ctypes.c_void_p(w.ctypes.data), N, K, ctypes.c_void_p(hi.ctypes.data),
               ctypes.c_void_p(lo.ctypes.data), byref(sh)))
    dev = Wt.device
    return (torch.from_numpy(hi.view(np.int16)).to(dev), torch.from_numpy(lo.view(np.int16)).to(dev), sh.value)


def split_weights_f16(Wt):
    """fp32 device weights -> (hi, lo) fp16-bit uint16 device tensors + power-of-two shift,
    through the library's own host splitter (asw_split_weights_f16)."""
    import ctypes
    import numpy as np
    w = np.ascontiguousarray(Wt.detach().cpu().numpy(), dtype=np.float32)
    hi = np.empty(w.size, dtype=np.uint16)
    lo = np.empty(w.size, dtype=np.uint16)
    sh = ctypes.c_int32()
    check(lib().asw_split_weights_f16(ctypes.c_void_p(w.ctypes.data), w.size, ctypes.c_void_p(hi.ctypes.data),
                                      ctypes.c_void_p(lo.ctypes.data), byref(sh)))
    dev = Wt.device
    return (torch.from_numpy(hi.view(np.int16)).to(dev), torch.from_numpy(lo.view(np.int16)).to(dev), sh.value)


def gn_glu(raw, stats, gamma, beta, eps=1e-5):
    B, T, C2 = raw.shape
    C = C2 // 2
    out = torch.empty((B, T, C), dtype=torch.float32, device=raw.device)
    check(lib().asw_gn_glu(ptr(_f32(raw)), ptr(_f32(stats)), stats.shape[1], ptr(_f32(gamma)), ptr(_f32(beta)),
                           B, T, C, eps, ptr(out), current_stream()))
    return out


def gn_finalize(stats, T, C, eps=1e-5):
    """Partial GroupNorm sums [B][n][4] -> (mean0, rstd0, mean1, rstd1) per batch item (asw_gn_finalize)."""
    B = stats.shape[0]
    mr = torch.empty((B, 4), dtype=torch.float32, device=stats.device)
    check(lib().asw_gn_finalize(ptr(_f32(stats)), stats.shape[1], B, T, C, eps, ptr(mr), current_stream()))
    return mr


def add_layernorm(x, resid, gamma, beta, eps=1e-5):
    rows, N = x.shape
    out = torch.empty_like(x)
    check(lib().asw_add_layernorm(ptr(_f32(x)), ptr(_f32(resid)), ptr(_f32(gamma)), ptr(_f32(beta)), rows, N, eps,
                                  ptr(out), current_stream()))
    return out


def attention(qkv, nhead, precision="f32"):
    B, L, d3 = qkv.shape
    d = d3 // 3
    ctx = torch.empty((B, L, d), dtype=torch.float32, device=qkv.device)
    check(lib().asw_attention_prec(ptr(_f32(qkv)), B, L, d, nhead, {"f32": 0, "f16x3": 1, "f16": 2}[precision], ptr(ctx),
                                   current_stream()))
    return ctx


def shift_stats(mix, offsets, circular=True):
    M, T = mix.shape
    N = offsets.shape[0]
    mean = torch.empty((N,), dtype=torch.float32, device=mix.device)
    std = torch.empty((N,), dtype=torch.float32, device=mix.device)
    check(lib().asw_shift_stats(ptr(_f32(mix)), M, T, ptr(offsets), N, int(circular), ptr(mean), ptr(std),
                                current_stream()))
    return mean, std


def shift_norm_preproc(mix, offsets, mean, std, w, b, T_pad, circular=True):
    M, T = mix.shape
    N = offsets.shape[0]
    C = w.shape[0]
    x0 = torch.empty((N, T_pad, C), dtype=torch.float32, device=mix.device)
    refn = torch.zeros((N, T_pad), dtype=torch.float32, device=mix.device)
    check(lib().asw_shift_norm_preproc(ptr(_f32(mix)), M, T, T_pad, ptr(offsets), N, int(circular), ptr(mean),
                                       ptr(std), ptr(_f32(w)), ptr(_f32(b)), C, ptr(x0), ptr(refn), T_pad,
                                       current_stream()))
    return x0, refn


def shift_norm_src(mix, offsets, mean, std, T_pad, circular=True):
    """asw_shift_norm_src_multi on one mixture: (src_hi, src_lo) [N][T_pad][8] fp16 planes and refn [N][T_pad]."""
    M, T = mix.shape
    N = offsets.shape[0]
    hi = torch.empty((N, T_pad, 8), dtype=torch.float16, device=mix.device)
    lo = torch.empty((N, T_pad, 8), dtype=torch.float16, device=mix.device)
    refn = torch.zeros((N, T_pad), dtype=torch.float32, device=mix.device)
    check(lib().asw_shift_norm_src_multi(ptr(_f32(mix)), M, T, T_pad, ptr(offsets), None, N, int(circular), ptr(mean),
                                         ptr(std), ptr(hi), ptr(lo), ptr(refn), T_pad, current_stream()))
    return hi, lo, refn


def overlap_add_unnorm(D, taps, hop, t, trim_left, trim_right, bias, mean=None, std=None):
    B, F, ldd = D.shape
    out = torch.empty((B, t), dtype=torch.float32, device=D.device)
    check(lib().asw_overlap_add_unnorm(ptr(_f32(D)), B, F, ldd, taps, hop, t, trim_left, trim_right, float(bias),
                                       ptr(mean), ptr(std), ptr(out), current_stream()))
    return out


def overlap_add_parts(Dp, taps, hop, t, trim_left, trim_right, bias, mean=None, std=None):
    """Dp [nparts][B][F][ldd] partial tap products (mask_path) -> out [B][t]."""
    nparts, B, F, ldd = Dp.shape
    out = torch.empty((B, t), dtype=torch.float32, device=Dp.device)
    check(lib().asw_overlap_add_parts(ptr(_f32(Dp)), nparts, B, F, ldd, taps, hop, t, trim_left, trim_right,
                                      float(bias), ptr(mean), ptr(std), ptr(out), current_stream()))
    return out


def mask_path(x, ref, ref_hop, enc_w, enc_b, byp_w, byp_b, dec_w, frames, stride, pad, precision="f16x3", scaled=False):
    """Fused mask path (asw_mask_path_f16x3; scaled=True: asw_mask_path_f16x3_scaled, every latent row brought into
    one fp16 binade before the split, "f16x3" only).  x [B][Tp][C] channels-last activations, ref [B][RL] padded
    reference rows (frame f reads ref[b][f*ref_hop + k]), enc_w [E][C][EK], byp_w [E][1][EKb], dec_w
    [E][1][EKd] torch-layout weights.  Returns the partial tap products [E/256][B][frames][64].
    precision: "f16x3" or the single-pass "f16"."""
    B, Tp, C = x.shape
    E, _, EK = enc_w.shape
    dev = x.device
    Wt = pack_conv_weight(enc_w).to(dev)
    fh, fl, sh = pack_fragments_f16(Wt, E, EK * C)
    wb = torch.zeros((E, 48), dtype=torch.float32)
    wb[:, :byp_w.shape[-1]] = byp_w[:, 0].cpu()
    bh, bl, bsh = pack_fragments_f16(wb.to(dev), E, 48)
    wd = torch.zeros((64, E), dtype=torch.float32)
    wd[:dec_w.shape[-1]] = dec_w[:, 0].t().cpu()
    dh, dl, dsh = pack_fragments_f16(wd.to(dev), 64, E)
    parts = torch.zeros((E // 256, B, frames, 64), dtype=torch.float32, device=dev)
    m = MaskPathArgs()
    a = m.enc
    a.A, a.bias = _f32(x).data_ptr(), (_f32(enc_b).data_ptr() if enc_b is not None else None)
    a.B, a.M_out, a.N, a.Cin, a.taps, a.stride, a.dil, a.pad = B, frames, E, C, EK, stride, 1, pad
    a.a_row_stride, a.a_batch_stride, a.a_len = C, Tp * C, Tp * C
    a.precision, a.w_shift, a.Wf_hi, a.Wf_lo = {"f16x3": 1, "f16": 2}[precision], sh, fh.data_ptr(), fl.data_ptr()
    m.ref, m.ref_batch_stride, m.ref_len, m.ref_hop = _f32(ref).data_ptr(), ref.shape[1], ref.shape[1], ref_hop
    m.byp_k, m.byp_taps, m.byp_shift = 48, byp_w.shape[-1], bsh
    m.byp_hi, m.byp_lo = bh.data_ptr(), bl.data_ptr()
    m.byp_bias = _f32(byp_b).data_ptr() if byp_b is not None else None
    m.dec_hi, m.dec_lo, m.dec_shift, m.dec_taps = dh.data_ptr(), dl.data_ptr(), dsh, dec_w.shape[-1]
    m.taps = parts.data_ptr()
    check((lib().asw_mask_path_f16x3_scaled if scaled else lib().asw_mask_path_f16x3)(byref(m), current_stream()))
    torch.cuda.current_stream().synchronize()
    return parts


def energies(y, window=12000):
    B, T = y.shape
    out = torch.empty((B, 2), dtype=torch.float64, device=y.device)
    check(lib().asw_energies(ptr(_f32(y)), B, T, window, None, ptr(out), current_stream()))   # scratch: ignored
    return out


def pair_sisdr(y):
    n, T = y.shape
    out = torch.empty((n, n), dtype=torch.float64, device=y.device)
    check(lib().asw_pair_sisdr(ptr(_f32(y)), n, T, ptr(out), current_stream()))
    return out


# ---- the two stages of the SRP-PHAT map (csrc/srp_kernels.hip) --------------------------------
def srp_cross_spectra(mix, twiddle, pair_i, pair_j, nbins, window, step, n_windows, nfft, hop, tol=1e-8):
    """DFT-GEMM + PHAT + frame-averaged cross-spectrum of every pair (asw_srp_cross_spectra).
    mix [M][T], twiddle [2*nb_pad][nfft] (srp._twiddles) -> cc [n_windows][nbins][P][2]."""
    M, T = mix.shape
    P = pair_i.shape[0]
    nb_pad = twiddle.shape[0] // 2
    assert twiddle.shape == (2 * nb_pad, nfft), "twiddle must be [2*nb_pad, nfft]"
    for t in (pair_i, pair_j):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == P, "pair tables: int32 [P]"
    F = lib().asw_srp_frames(window, nfft, hop)
    xf = torch.empty((M, max(F, 1), 2 * nb_pad), dtype=torch.float32, device=mix.device)
    # NaN-filled, so that an entry the kernel leaves unwritten shows in a comparison whatever the allocator held
    cc = torch.full((n_windows, nbins, P, 2), float("nan"), dtype=torch.float32, device=mix.device)
    check(lib().asw_srp_cross_spectra(ptr(_f32(mix)), M, T, window, step, n_windows, nfft, hop, nbins, nb_pad, tol,
                                      ptr(_f32(twiddle)), ptr(pair_i), ptr(pair_j), P, ptr(xf), ptr(cc),
                                      current_stream()))
    return cc


def srp_map(cc, tau, omega, pair_i, pair_j):
    """Steered-response map, running maximum over the windows of cc starting from zeros (asw_srp_map).
    cc [n_windows][nbins][P][2], tau [G][M] and omega [nbins] float64 -> [G]."""
    n_windows, nbins, P, _ = cc.shape
    G, M = tau.shape
    for t, dt, n in ((tau, torch.float64, G * M), (omega, torch.float64, nbins), (pair_i, torch.int32, P),
                     (pair_j, torch.int32, P)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == n, "srp_map: operand dtype / size"
    part = torch.empty((8 * 8 * G,), dtype=torch.float32, device=cc.device)
    out = torch.empty((G,), dtype=torch.float32, device=cc.device)
    check(lib().asw_srp_map(ptr(_f32(cc)), n_windows, nbins, P, ptr(tau), G, M, ptr(omega), ptr(pair_i), ptr(pair_j),
                            ptr(part), ptr(out), current_stream()))
    return out


# ---- kernels of the joint separation network (csrc/sep_kernels.hip) --------------------------
def joint_shift_stats(mix, offsets):
    """mean / unbiased std of the all-channel average of the S*M zero-fill shifted channels."""
    M, T = mix.shape
    S = offsets.shape[0]
    scratch = torch.empty((lib().asw_joint_shift_stats_scratch_doubles(),), dtype=torch.float64, device=mix.device)
    mean = torch.empty((S,), dtype=torch.float32, device=mix.device)
    std = torch.empty((S,), dtype=torch.float32, device=mix.device)
    check(lib().asw_joint_shift_stats(ptr(_f32(mix)), M, T, ptr(offsets), S, ptr(scratch), ptr(mean), ptr(std),
                                      current_stream()))
    return mean, std


def _group_tables(counts):
    """host tables of a ragged call: bounds [G+1] and the item of each group, over the items that hold a sequence"""
    import ctypes
    bounds, items = [0], []
    for k, c in enumerate(counts):
        if int(c) > 0:
            bounds.append(bounds[-1] + int(c))
            items.append(k)
    return (ctypes.c_int32 * len(bounds))(*bounds), (ctypes.c_int32 * max(1, len(items)))(*items), len(items)


def joint_shift_stats_groups(mix_stack, offsets, counts):
    """``joint_shift_stats`` per item of a ragged call: mix_stack [K,M,T], offsets [N,M-1] item after item, counts [K]
    -> mean, std [N] (one value per item, on each of its sequences)."""
    K, M, T = mix_stack.shape
    N = offsets.shape[0]
    assert len(counts) == K and sum(int(c) for c in counts) == N and all(int(c) >= 0 for c in counts)
    assert offsets.is_cuda and offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.shape[1] == M - 1
    bounds, items, G = _group_tables(counts)
    scratch = torch.empty((max(1, G) * lib().asw_joint_shift_stats_scratch_doubles(),), dtype=torch.float64,
                          device=mix_stack.device)
    mean = torch.empty((N,), dtype=torch.float32, device=mix_stack.device)
    std = torch.empty((N,), dtype=torch.float32, device=mix_stack.device)
    check(lib().asw_joint_shift_stats_groups(ptr(_f32(mix_stack)), M, T, ptr(offsets), bounds, G, items, ptr(scratch),
                                             ptr(mean), ptr(std), current_stream()))
    return mean, std


def add_layernorm2(x, y=None, alpha=1.0, gamma=None, beta=None, eps=1e-5, act=0, want_sum=False, want_ln=True):
    rows, N = x.shape
    s = torch.empty_like(x) if want_sum else None
    o = torch.empty_like(x) if want_ln else None
    check(lib().asw_add_layernorm2(ptr(_f32(x)), ptr(y), float(alpha), ptr(gamma), ptr(beta), rows, N, eps, act, ptr(s),
                                   ptr(o), current_stream()))
    return s, o


def glu_rows(raw):
    rows, C2 = raw.shape
    out = torch.empty((rows, C2 // 2), dtype=torch.float32, device=raw.device)
    check(lib().asw_glu_rows(ptr(_f32(raw)), rows, C2 // 2, ptr(out), current_stream()))
    return out


def dwconv_ln_swish(u, w, bias, gamma, beta, eps=1e-5):
    """u [BS, L, d]; w torch depthwise weight [d, 1, K]."""
    BS, L, d = u.shape
    K = w.shape[-1]
    wT = w.reshape(d, K).t().contiguous()
    out = torch.empty_like(u)
    check(lib().asw_dwconv_ln_swish(ptr(_f32(u)), ptr(_f32(wT)), ptr(_f32(bias)), ptr(_f32(gamma)), ptr(_f32(beta)),
                                    BS, L, d, K, eps, ptr(out), current_stream()))
    return out


def relpos_attention(qkv, P, bias_u, bias_v, nhead, scale):
    BS, L, d3 = qkv.shape
    d = d3 // 3
    ctx = torch.empty((BS, L, d), dtype=torch.float32, device=qkv.device)
    check(lib().asw_relpos_attention(ptr(_f32(qkv)), ptr(_f32(P)), ptr(_f32(bias_u)), ptr(_f32(bias_v)), BS, L, d, nhead,
                                     float(scale), ptr(ctx), current_stream()))
    return ctx


def inter_attention(qkv, nhead):
    NB, S, L, d3 = qkv.shape
    d = d3 // 3
    ctx = torch.empty((NB, S, L, d), dtype=torch.float32, device=qkv.device)
    check(lib().asw_inter_attention(ptr(_f32(qkv)), NB, S, L, d, nhead, ptr(ctx), current_stream()))
    return ctx


def inter_attention_groups(qkv, counts, nhead, out=None):
    """``inter_attention`` over groups of different sizes: qkv [N,L,3d] with counts[g] consecutive sequences in group g
    (zeros are left out) -> ctx [N,L,d].  ``out``: write into this tensor (tests)."""
    N, L, d3 = qkv.shape
    d = d3 // 3
    assert sum(int(c) for c in counts) == N and all(int(c) >= 0 for c in counts)
    bounds, _items, G = _group_tables(counts)
    ctx = torch.empty((N, L, d), dtype=torch.float32, device=qkv.device) if out is None else out
    assert ctx.shape == (N, L, d)
    check(lib().asw_inter_attention_groups(ptr(_f32(qkv)), bounds, G, L, d, nhead, ptr(_f32(ctx)), current_stream()))
    return ctx


def _host_i32(values):
    import ctypes
    flat = [int(v) for v in values]
    return (ctypes.c_int32 * max(1, len(flat)))(*flat)


def frame_blocks(mix, starts, T, out=None):
    """mix [M,Ttot] -> the blocks [K,M,T] that start at ``starts`` (host integers), zero past the end
    (``longform.frame_f64``).  ``out``: write into this tensor (tests)."""
    M, Ttot = mix.shape
    K = len(starts)
    blocks = torch.empty((K, M, int(T)), dtype=torch.float32, device=mix.device) if out is None else out
    assert blocks.shape == (K, M, int(T))
    check(lib().asw_frame_blocks(ptr(_f32(mix)), M, Ttot, _host_i32(starts), K, int(T), ptr(_f32(blocks)), current_stream()))
    return blocks


def stitch_blocks(rows, taper, starts, row_of, Ttot, out=None):
    """The normalised overlap-add of ``longform.stitch_f64``: rows [N,T] float32, taper [T] float64 (device), starts [K] and
    row_of [K][S] host integers -> [S,Ttot] float32.  ``out``: write into this tensor (tests)."""
    N, T = rows.shape
    K = len(starts)
    S = len(row_of[0])
    assert len(row_of) == K and all(len(r) == S for r in row_of)
    assert taper.is_cuda and taper.dtype == torch.float64 and taper.is_contiguous() and taper.shape == (T,)
    res = torch.empty((S, int(Ttot)), dtype=torch.float32, device=rows.device) if out is None else out
    assert res.shape == (S, int(Ttot))
    check(lib().asw_stitch_blocks(ptr(_f32(rows)), N, ptr(taper), _host_i32(starts), _host_i32(v for r in row_of for v in r), K, S,
                                  T, int(Ttot), ptr(_f32(res)), current_stream()))
    return res


def _ws_f64(nbytes, device):
    return torch.empty(((int(nbytes) + 7) // 8,), dtype=torch.float64, device=device)


def stft(x, out=None):
    """x [R,N] float32 -> complex128 [R,1025,F], the STFT of ``oracle_masks.stft_f64``.  ``out``: write into this
    tensor (tests)."""
    from .oracle_masks import NBINS, frame_count
    R, N = x.shape
    F = frame_count(N)
    z = torch.empty((R, NBINS, F), dtype=torch.complex128, device=x.device) if out is None else out
    assert z.shape == (R, NBINS, F) and z.dtype == torch.complex128 and z.is_cuda and z.is_contiguous()
    check(lib().asw_stft(ptr(_f32(x)), R, N, ptr(z), current_stream()))
    return z


def istft(z, N, out=None):
    """z [R,1025,F] complex128 -> [R,N] float64, the inverse STFT of ``oracle_masks.istft_f64``.  ``out``: write into
    this tensor (tests)."""
    R, _nb, F = z.shape
    assert z.is_cuda and z.dtype == torch.complex128 and z.is_contiguous() and _nb == 1025
    res = torch.empty((R, int(N)), dtype=torch.float64, device=z.device) if out is None else out
    assert res.shape == (R, int(N)) and res.dtype == torch.float64 and res.is_cuda and res.is_contiguous()
    nbytes = lib().asw_istft_workspace_bytes(R, F)
    if nbytes == 0:
        check(-1)
    ws = _ws_f64(nbytes, z.device)
    check(lib().asw_istft(ptr(z), R, F, int(N), ptr(res), ptr(ws), nbytes, current_stream()))
    return res


ORACLE_KINDS = {"irm": 0, "ibm": 1}            # ASW_ORACLE_IRM, ASW_ORACLE_IBM


def oracle_masks(mix, ref, counts, lengths, kind, alpha=1.0, theta=0.5, out=None):
    """The oracle mask estimates of K items in one call (``oracle_masks.irm_f64`` / ``ibm_f64`` per item): mix [K,T] and
    ref [sum counts,T] float32, ``counts`` and ``lengths`` host integers -> [sum counts,T] float64, row j of item k zero
    beyond lengths[k].  ``out``: write into this tensor (tests)."""
    K, T = mix.shape
    assert len(counts) == K and len(lengths) == K and ref.shape == (sum(int(c) for c in counts), T)
    res = torch.empty((ref.shape[0], T), dtype=torch.float64, device=mix.device) if out is None else out
    assert res.shape == (ref.shape[0], T) and res.dtype == torch.float64 and res.is_cuda and res.is_contiguous()
    c, n = _host_i32(counts), _host_i32(lengths)
    nbytes = lib().asw_oracle_masks_workspace_bytes(c, n, K)
    if nbytes == 0:
        check(-1)
    ws = _ws_f64(nbytes, mix.device)
    check(lib().asw_oracle_masks(ptr(_f32(mix)), ptr(_f32(ref)) if ref.shape[0] else None, c, n, K, T, ORACLE_KINDS[kind],
                                 float(alpha), float(theta), ptr(res) if ref.shape[0] else None, ptr(ws), nbytes,
                                 current_stream()))
    return res


def _host_f64(a, shape):
    import numpy as np
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    assert a.shape == tuple(shape), f"shape {a.shape}, expected {tuple(shape)}"
    return a


def room_rir(rooms, absorption, max_orders, src, mics, counts, fs, length, device=None, out=None):
    """The image-source responses of K shoebox scenes in one call (``roomsim.rir_f64``): rooms [K,3], absorption [K],
    src [sum counts,3] and mics [K,M,3] host float64 arrays, ``max_orders`` and ``counts`` host integers -> float64
    [sum counts,M,length] on ``device`` (the current one by default).  ``out``: write into this tensor (tests)."""
    K = len(counts)
    NS = sum(int(c) for c in counts)
    import numpy as np
    M = np.shape(mics)[1]
    rooms, absorption, src = _host_f64(rooms, (K, 3)), _host_f64(absorption, (K,)), _host_f64(src, (NS, 3))
    mics = _host_f64(mics, (K, M, 3))
    assert len(max_orders) == K
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if out is None else out.device
    res = torch.empty((NS, M, int(length)), dtype=torch.float64, device=device) if out is None else out
    assert res.shape == (NS, M, int(length)) and res.dtype == torch.float64 and res.is_cuda and res.is_contiguous()
    nbytes = lib().asw_room_rir_workspace_bytes(K, M, NS)
    if nbytes == 0:
        check(-1)
    with torch.cuda.device(res.device):
        ws = _ws_f64(nbytes, res.device)
        check(lib().asw_room_rir(rooms.ctypes.data, absorption.ctypes.data, _host_i32(max_orders), src.ctypes.data, mics.ctypes.data,
                                 _host_i32(counts), K, M, float(fs), int(length), ptr(res), ptr(ws), nbytes, current_stream()))
    return res


def room_convolve(dry, rir, counts, out=None):
    """dry [sum counts,T] float32 through rir [sum counts,M,length] float64 (``roomsim.convolve_f64``) -> (premix
    [sum counts,M,T], mix [K,M,T]) float64, mix the sum of a scene's premix rows in source order.  ``out``: the pair of
    tensors to write into (tests)."""
    NS, T = dry.shape
    _ns, M, length = rir.shape
    K = len(counts)
    assert _ns == NS == sum(int(c) for c in counts)
    assert rir.is_cuda and rir.dtype == torch.float64 and rir.is_contiguous()
    premix, mix = (torch.empty((NS, M, T), dtype=torch.float64, device=dry.device),
                   torch.empty((K, M, T), dtype=torch.float64, device=dry.device)) if out is None else out
    for t, shape in ((premix, (NS, M, T)), (mix, (K, M, T))):
        assert t.shape == shape and t.dtype == torch.float64 and t.is_cuda and t.is_contiguous()
    c = _host_i32(counts)
    nbytes = lib().asw_room_convolve_workspace_bytes(c, K, M, length, T)
    if nbytes == 0:
        check(-1)
    ws = _ws_f64(nbytes, dry.device)
    check(lib().asw_room_convolve(ptr(_f32(dry)) if NS else None, ptr(rir) if NS else None, c, K, M, length, T,
                                  ptr(premix) if NS else None, ptr(mix), ptr(ws), nbytes, current_stream()))
    return premix, mix


def _host_i64(values):
    import ctypes
    flat = [((int(v) + 2 ** 63) % 2 ** 64) - 2 ** 63 for v in values]         # 64-bit keys, as signed words
    return (ctypes.c_int64 * max(1, len(flat)))(*flat)


def _host_f64_list(values):
    import ctypes
    flat = [float(v) for v in values]
    return (ctypes.c_double * max(1, len(flat)))(*flat)


def colored_noise(key, rows, T, exponent=1.0, max_rows_per_pass=0, device=None, out=None):
    """Power-law noise rows (``train_data.colored_noise_f64``) -> float64 [rows,T] on ``device``.  ``key``: one integer for
    every row, or one per row; ``rows``: a count (rows 0..rows-1 of the key) or the list of row indices.  Rows are
    processed ``max_rows_per_pass`` at a time (0: what fits 256 MiB of workspace); the bytes do not depend on it.
    ``out``: write into this tensor (tests)."""
    ids = list(range(rows)) if isinstance(rows, int) else [int(r) for r in rows]
    keys = [int(key)] * len(ids) if isinstance(key, int) else [int(k) for k in key]
    assert len(keys) == len(ids)
    n = len(ids)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if out is None else out.device
    res = torch.empty((n, int(T)), dtype=torch.float64, device=device) if out is None else out
    assert res.shape == (n, int(T)) and res.dtype == torch.float64 and res.is_cuda and res.is_contiguous()
    nbytes = lib().asw_colored_noise_workspace_bytes(n, int(T), int(max_rows_per_pass))
    if nbytes == 0:
        check(-1)
    with torch.cuda.device(res.device):
        ws = _ws_f64(nbytes, res.device)
        check(lib().asw_colored_noise(_host_i64(keys), _host_i32(ids), n, int(T), float(exponent), int(max_rows_per_pass), ptr(res),
                                      ptr(ws), nbytes, current_stream()))
    return res


def train_batch(mix, item_mix, shifts, counts, pink_level, white_level, white_key, pink=None, dtype=torch.float32, out=None):
    """mix [K,M,T] float32 -> [I,S_max*M,T]: block s of item i is mixture ``item_mix[i]`` rolled by ``shifts[i][s]`` (host
    integers [I][S_max][M]) for s < ``counts[i]`` and zero beyond, plus ``white_level[i]`` times inline Philox normals
    under ``white_key[i]`` plus ``pink_level[i]`` times ``pink`` [I,S_max*M,T] float64 (``colored_noise``; may be None when
    every pink level is zero), summed in float64 and rounded once (``train_data.train_batch_f64``).  ``dtype``:
    torch.float32, or torch.float64 for the unrounded sum (tests).  ``out``: write into this tensor (tests)."""
    import numpy as np
    K, M, T = mix.shape
    sh = np.ascontiguousarray(np.asarray(shifts, dtype=np.int32))
    n_items = len(item_mix)
    assert sh.ndim == 3 and sh.shape[0] == n_items and sh.shape[2] == M, f"shifts {sh.shape}: expected [{n_items}][S_max][{M}]"
    S = sh.shape[1]
    assert len(counts) == len(pink_level) == len(white_level) == len(white_key) == n_items
    assert dtype in (torch.float32, torch.float64)
    if pink is not None:
        assert pink.shape == (n_items, S * M, T) and pink.dtype == torch.float64 and pink.is_contiguous() and pink.device == mix.device
    res = torch.empty((n_items, S * M, T), dtype=dtype, device=mix.device) if out is None else out
    assert res.shape == (n_items, S * M, T) and res.dtype == dtype and res.is_cuda and res.is_contiguous()
    nbytes = lib().asw_train_batch_workspace_bytes(n_items, S, M)
    if nbytes == 0:
        check(-1)
    with torch.cuda.device(mix.device):
        ws = _ws_f64(nbytes, mix.device)
        check(lib().asw_train_batch(ptr(_f32(mix)), K, M, T, n_items, S, _host_i32(item_mix), sh.ctypes.data, _host_i32(counts),
                                    _host_f64_list(pink_level), _host_f64_list(white_level), _host_i64(white_key), ptr(pink), ptr(res),
                                    int(dtype == torch.float64), ptr(ws), nbytes, current_stream()))
    return res


def train_losses(est, gt, out=None):
    """est, gt [N,T] float32 -> float64 [N,4]: mean |e - g|, the negative SNR, the negative SI-SDR and max |g| of every
    row (``train_data.row_losses_f64``); ``train_data.loss_from_rows`` combines them into the scalar of a loss name.
    ``out``: write into this tensor (tests)."""
    N, T = est.shape
    assert gt.shape == est.shape and gt.device == est.device
    res = torch.empty((N, 4), dtype=torch.float64, device=est.device) if out is None else out
    assert res.shape == (N, 4) and res.dtype == torch.float64 and res.is_cuda and res.is_contiguous()
    with torch.cuda.device(est.device):
        check(lib().asw_train_losses(ptr(_f32(est)), ptr(_f32(gt)), N, T, ptr(res), current_stream()))
    return res


def _host_i64_array(values):
    import numpy as np
    return np.ascontiguousarray(np.asarray(list(values), dtype=np.int64).reshape(-1))


_voice_filters = {}


def voice_filter(up, down, device):
    """The resampler's filter table (``voiceprep.resample_filter``) on ``device``, built once per ratio and device."""
    from . import voiceprep
    key = voiceprep.reduced(up, down) + (str(device),)
    if key not in _voice_filters:
        _voice_filters[key] = torch.from_numpy(voiceprep.resample_filter(up, down)).to(device)
    return _voice_filters[key]


def voice_resample(x, row_offset, row_len, up, down, win_begin, win_len, T_out, h=None, dtype=torch.float32, out=None):
    """The rows ``x[row_offset[r] : row_offset[r] + row_len[r]]`` of the packed float32 ``x``, resampled by ``up / down``
    (``voiceprep.resample_poly_f64``) -> [n,T_out]: row r holds the ``win_len[r]`` resampled samples from ``win_begin[r]``
    on and zeros past them or past the row's end.  The tables are host integers; ``h``: the filter table on the device
    (``voice_filter`` by default).  ``dtype``: torch.float32 (the float64 sum rounded once) or torch.float64.  ``out``:
    write into this tensor (tests)."""
    n = len(row_len)
    assert len(row_offset) == len(win_begin) == len(win_len) == n
    assert x.dim() == 1 and dtype in (torch.float32, torch.float64)
    if h is None:
        h = voice_filter(up, down, x.device)
    assert h.is_cuda and h.dtype == torch.float64 and h.is_contiguous() and h.dim() == 1 and h.device == x.device
    res = torch.empty((n, int(T_out)), dtype=dtype, device=x.device) if out is None else out
    assert res.shape == (n, int(T_out)) and res.dtype == dtype and res.is_cuda and res.is_contiguous()
    nbytes = lib().asw_voice_resample_workspace_bytes(n)
    if nbytes == 0:
        check(-1)
    off, wb = _host_i64_array(row_offset), _host_i64_array(win_begin)
    with torch.cuda.device(x.device):
        ws = _ws_f64(nbytes, x.device)
        check(lib().asw_voice_resample(ptr(_f32(x)), x.shape[0], off.ctypes.data, _host_i32(row_len), n, int(up), int(down), ptr(h),
                                       h.shape[0], wb.ctypes.data, _host_i32(win_len), int(T_out), ptr(res),
                                       int(dtype == torch.float64), ptr(ws), nbytes, current_stream()))
    return res


def voice_trim(x, row_offset, row_len, top_db=18.0, out=None):
    """``voiceprep.trim_f64`` of every row of the packed float32 ``x`` -> (bounds [n,2] int32 = begin and end of the
    non-silent span, stats [n,2] float64 = the peak frame mean square and the variance of the span).  The tables are
    host integers.  ``out``: the pair of tensors to write into (tests)."""
    n = len(row_len)
    assert len(row_offset) == n and x.dim() == 1
    bounds, stats = (torch.empty((n, 2), dtype=torch.int32, device=x.device),
                     torch.empty((n, 2), dtype=torch.float64, device=x.device)) if out is None else out
    for t, dt in ((bounds, torch.int32), (stats, torch.float64)):
        assert t.shape == (n, 2) and t.dtype == dt and t.is_cuda and t.is_contiguous()
    max_len = max([int(v) for v in row_len], default=0)
    nbytes = lib().asw_voice_trim_workspace_bytes(n, max_len)
    if nbytes == 0:
        check(-1)
    off = _host_i64_array(row_offset)
    with torch.cuda.device(x.device):
        ws = _ws_f64(nbytes, x.device)
        check(lib().asw_voice_trim(ptr(_f32(x)), x.shape[0], off.ctypes.data, _host_i32(row_len), n, max_len,
                                   10.0 ** (-float(top_db) / 10.0), ptr(bounds), ptr(stats), ptr(ws), nbytes, current_stream()))
    return bounds, stats


def f16x3_overflow_count(reset=True) -> int:
    """Threads of f16x3 launches that produced an activation beyond the fp16 range since the last
    reset (asw_f16x3_overflow_count); 0 means no later GEMM clipped its input."""
    import ctypes
    c = ctypes.c_int32()
    check(lib().asw_f16x3_overflow_count(int(reset), byref(c)))
    return int(c.value) & 0xFFFFFFFF
