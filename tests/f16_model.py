"""A CPU model of the arithmetic of the split-fp16 matrix kernels (csrc/f16x3_tile.h: mma3, split4t; precision "f16x3"
and single-pass "f16"), in numpy.  Plain module: no fixtures.

The operand split is deterministic, and a product of two fp16 numbers is exact in float64.  So "split as the kernel
splits, then exact products, summed in float64" says what a kernel of either mode should produce; a correct kernel
differs from it only by its fp32 accumulation and its fp32 epilogue.  That is a far smaller distance than the one
between the arithmetic and the truth (2^-11 per operand in the one-term mode), so a kernel held to this model is held
about a thousand times tighter in "f16" and tens of times tighter in "f16x3" than one held to float64 of the inputs.

Two layers:
  splits and products   rtz16 / rn16 / split_act (csrc/mfma_util.h: split4, split4_rn), split_attn (csrc/attention.hip:
                        split4h; its users are in tests/attention_cases.py), split_np / split_w
                        (csrc/asw_common.cpp: asw_split_weights_f16), accumulate (the three terms of mma3)
  fused operations      conv_layer (im2col, + bias, ReLU / Swish, (x + x2), * mul, residual, LayerNorm), gn_glu,
                        stats4, stack (the hand-over between fused layers), up_tail (UpFeed)

accumulate(acc="f32") is the float32 stand-in: the same exact products, 16 k at a time as one MFMA takes them, added
to a float32 accumulator in a given order of k.  It is not a model of anything; its distance from the float64 model
sizes the bars (bars()).

Which residual a kernel adds (conv_layer(resid=...)):
  "image"    the layer's own input read back from the LDS image as float(hi) + float(lo): resstack64 in every form
             (csrc/resstack.hip, finish_rows: `v += (float)rh[j] + (float)rl[j]`) and resconv16 at C = 64
             (csrc/resconv.hip, `if constexpr (C == 64)`: rpre = hi + lo)
  an array   the fp32 tensor: resconv16 at C >= 128 and the generic tiles (csrc/gemm_epilogue.h, `p.resid + obase`)
"""
import numpy as np

F16_MAX = np.float32(65504.0)
NTERM = {"f16x3": 3, "f16": 1}


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------------------- splits and products
def rn16(x):
    """fp32 -> fp16, round to nearest even, clamped to +-65504 first (finite overflow saturates)"""
    return np.clip(_f32(x), -F16_MAX, F16_MAX).astype(np.float16)


def rtz16(x):
    """fp32 -> fp16 toward zero; finite overflow saturates at +-65504 (v_cvt_pkrtz_f16_f32)"""
    c = np.clip(_f32(x), -F16_MAX, F16_MAX)
    h = c.astype(np.float16)
    away = np.abs(h.astype(np.float32)) > np.abs(c)            # nearest went away from zero: one step back
    return np.where(away, np.nextafter(h, np.float16(0.0)), h).astype(np.float16)


def split_act(x, nterm):
    """The activation split: hi truncated (three terms, split4) or rounded to nearest (one term, split4_rn: nothing
    catches the remainder there), lo = rtz(x - float(hi)) in both.  -> (hi, lo) as float16"""
    x = _f32(x)
    hi = rtz16(x) if nterm == 3 else rn16(x)
    with np.errstate(over="ignore", invalid="ignore"):
        lo = rtz16(x - hi.astype(np.float32))
    return hi, lo


def split_attn(x):
    """The split of attention_mfma16_kernel (csrc/attention.hip, split4h): hi truncated, lo = the remainder ROUNDED TO
    NEAREST.  -> float64(hi) + float64(lo), the value the f16 MFMAs multiply"""
    x = _f32(x)
    hi = rtz16(x)
    with np.errstate(over="ignore", invalid="ignore"):
        lo = rn16(x - hi.astype(np.float32))
    return hi.astype(np.float64) + lo.astype(np.float64)


def split_np(w):
    """shift = 11 - exponent of max|w| (frexp), clamped to +-24, 0 for all-zero weights; scale, clamp to the fp16
    range; hi = float16(c), lo = float16(c - float32(hi)), as uint16 bit patterns."""
    w = np.asarray(w, dtype=np.float32).ravel()
    mx = np.float32(np.max(np.abs(w)))
    shift = 0
    if mx > 0:
        shift = int(np.clip(11 - int(np.frexp(mx)[1]), -24, 24))
    c = np.clip(w * np.float32(2.0 ** shift), np.float32(-65504.0), np.float32(65504.0)).astype(np.float32)
    hi = c.astype(np.float16)
    lo = (c - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16), shift


def split_w(w):
    """split_np of a weight matrix -> (hi, lo) in float64, in the pre-scaled units the MFMA sees, and the shift"""
    w = _f32(w)
    hi, lo, shift = split_np(w)
    return (hi.view(np.float16).astype(np.float64).reshape(w.shape), lo.view(np.float16).astype(np.float64).reshape(w.shape),
            shift)


def accumulate(xh, xl, wh, wl, nterm, acc="f64", korder=1):
    """x_lo w_hi + x_hi w_lo + x_hi w_hi (one term: the last only) of xh, xl [R][K] and wh, wl [N][K], all float64
    holding fp16 values.  acc = "f64": summed in float64.  acc = "f32": the stand-in -- per 16 k the exact sum of a
    term's products is added to a float32 accumulator, terms inner in mma3's order, k-steps ascending (korder = 1)
    or descending (-1); the result holds float32 values."""
    if acc == "f64":
        if nterm == 3:
            return xl @ wh.T + xh @ wl.T + xh @ wh.T
        return xh @ wh.T
    R, K = xh.shape
    assert K % 16 == 0
    a = np.zeros((R, wh.shape[0]), dtype=np.float32)
    for ks in list(range(K // 16))[::korder]:
        s = slice(ks * 16, ks * 16 + 16)
        terms = ((xl, wh), (xh, wl), (xh, wh)) if nterm == 3 else ((xh, wh),)
        for x, w in terms:
            a = (a.astype(np.float64) + x[:, s] @ w[:, s].T).astype(np.float32)
    return a.astype(np.float64)


# ---------------------------------------------------------------------------------------------- fused operations
def im2col(x, taps, stride, dil, pad, M_out):
    """x [B][T][C] -> [B][M_out][taps * C] (tap-major, channel fastest: ops.pack_conv_weight), zeros outside"""
    B, T, C = x.shape
    right = max(0, (M_out - 1) * stride - pad + (taps - 1) * dil + 1 - T)
    xp = np.zeros((B, pad + T + right, C), dtype=x.dtype)
    xp[:, pad:pad + T] = x
    cols = [xp[:, j * dil: j * dil + (M_out - 1) * stride + 1: stride] for j in range(taps)]
    return np.concatenate(cols, axis=2)


def layer_norm(y, gamma, beta, eps):
    m = y.mean(-1, keepdims=True)
    v = ((y - m) ** 2).mean(-1, keepdims=True)
    return (y - m) / np.sqrt(v + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def conv_layer(x, w, nterm, taps=1, stride=1, dil=1, pad=0, M_out=None, bias=None, act=0, x2=None, mul=None, resid=None,
               ln=None, eps=1e-5, acc="f64", korder=1):
    """One GEMM-class launch.  x [B][T][Cin] fp32 ((x + x2) in fp32 first, the A2 operand), w [N][taps * Cin] fp32;
    act 0 none / 1 ReLU / 2 Swish; resid "image" (hi + lo of this layer's input), an fp32 array [B][M_out][N], or
    None; ln = (gamma, beta).  Everything after the products in float64.  nterm = 0: float64 of the unsplit operands,
    the truth the arithmetic is measured against.  -> [B][M_out][N] float64"""
    if nterm == 0:                                   # the truth: the same operation with nothing split or rounded
        xh = np.asarray(x, np.float64) + (0.0 if x2 is None else np.asarray(x2, np.float64))
        xl, wh, wl, shift = np.zeros_like(xh), np.asarray(w, np.float64), None, 0
        x = xh
    else:
        x = _f32(x)
        if x2 is not None:
            x = x + _f32(x2)
        hi, lo = split_act(x, nterm)
        xh, xl = hi.astype(np.float64), lo.astype(np.float64)
        wh, wl, shift = split_w(w)
    B, T, _ = x.shape
    M_out = T if M_out is None else M_out
    N, K = wh.shape
    ah = im2col(xh, taps, stride, dil, pad, M_out).reshape(B * M_out, K)
    al = im2col(xl, taps, stride, dil, pad, M_out).reshape(B * M_out, K)
    y = accumulate(ah, al, wh, wl, nterm, acc, korder).reshape(B, M_out, N) * 2.0 ** -shift
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if act == 1:
        y = np.maximum(y, 0.0)
    elif act == 2:
        y = y / (1.0 + np.exp(-y))
    if isinstance(resid, str):
        assert resid == "image" and y.shape == x.shape
        y = y + (xh + xl)
    elif resid is not None:
        y = y + np.asarray(resid, np.float64)
    if mul is not None:
        y = y * np.asarray(mul, np.float64)
    if ln is not None:
        y = layer_norm(y, ln[0], ln[1], eps)
    return y


def gn_glu(raw, mr, gamma, beta):
    """GroupNorm(2) + GLU of raw [B][T][value C | gate C] with finalised statistics mr [B][(mean0, rstd0, mean1,
    rstd1)], the expression of asw::gn_glu_value in float64.  The kernels split the fp32 value of that expression;
    its sigmoid runs on the hardware's approximate exp2 / rcp, which no CPU reproduces to the bit, so the GPU tests
    take the fp32 tensor to split from the kernel's side output and hold that tensor to this function."""
    raw, mr = np.asarray(raw, np.float64), np.asarray(mr, np.float64)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    C = raw.shape[-1] // 2
    a = (raw[..., :C] - mr[:, None, None, 0]) * mr[:, None, None, 1] * gamma[:C] + beta[:C]
    g = (raw[..., C:] - mr[:, None, None, 2]) * mr[:, None, None, 3] * gamma[C:] + beta[C:]
    return a / (1.0 + np.exp(-g))


def stats4(y, chan_mod):
    """The four GroupNorm partial sums of y [B][M][N], summed over a batch item: (sum, sum of squares) of the
    channels with n % chan_mod < chan_mod / 2, then of the others.  -> [B][4] float64"""
    y = np.asarray(y, np.float64)
    second = (np.arange(y.shape[-1]) % chan_mod) >= chan_mod // 2
    a, b = y[..., ~second], y[..., second]
    return np.stack([a.sum((1, 2)), (a ** 2).sum((1, 2)), b.sum((1, 2)), (b ** 2).sum((1, 2))], axis=1)


def ulp_nudge(x, rng, ulps=2):
    """float32 x moved by a random whole number of ulps in [-ulps, ulps] (zeros stay)"""
    x = _f32(x)
    k = rng.integers(-ulps, ulps + 1, size=x.shape).astype(np.int32)
    bits = x.view(np.int32)
    out = (bits + np.where(bits >= 0, k, -k)).view(np.float32)          # sign-magnitude: the same step on either sign
    return np.where(x == 0, x, out).astype(np.float32)


def stack(x, layers, nterm, taps=7, eps=1e-5, acc="f64", korder=1, nudge=None):
    """Residual layers LN(ReLU(conv(x) + b) + x) in a row, as resstack64 fuses them: each layer's output is rounded
    to fp32 and split again for the next (csrc/resstack.hip, hand_over), the residual is the image's hi + lo.
    layers: [(w [64][taps * 64] fp32, bias, gamma, beta, dil)].  nudge: a numpy Generator -- every hand-over is
    moved by up to +-2 fp32 ulps (the experiment that sizes the one-term chains' bar).  -> float64"""
    cur = x
    y = None
    for i, (w, b, g, be, d) in enumerate(layers):
        y = conv_layer(cur, w, nterm, taps=taps, dil=d, pad=d * (taps - 1) // 2, bias=b, act=1, resid="image", ln=(g, be),
                       eps=eps, acc=acc, korder=korder)
        cur = y.astype(np.float32) if nterm else y
        if nudge is not None and i + 1 < len(layers):
            cur = ulp_nudge(cur, nudge)
    return y


def up_tail(y, skip, up_wt, up_bias, nterm=3, acc="f64", korder=1):
    """UpFeed: (fp32 stack output + skip) in fp32, split, one-tap GEMM with up_wt [256][64] + bias (the order of the
    16 channels inside a k-step, asw_up_feed_kperm, does not enter: a k-step's products are summed exactly)"""
    return conv_layer(np.asarray(y).astype(np.float32), up_wt, nterm, bias=up_bias, x2=skip, acc=acc, korder=korder)


# ---------------------------------------------------------------------------------------------- measures and bars
def measures(got, want):
    """(relative L2 over the tensor, worst row: the row's error norm over that row's norm in `want`, the rows of
    all batch items pooled)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    g, w = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    e = np.linalg.norm(g - w, axis=1)
    return float(np.linalg.norm(e) / np.linalg.norm(w)), float(np.max(e / np.maximum(np.linalg.norm(w, axis=1), 1e-300)))


BAR_FACTOR = 4.0


def bars(fn):
    """fn(acc, korder) -> output.  -> (model, (bar_l2, bar_row)): the float64 model and BAR_FACTOR x its distance from
    the float32 stand-in, the larger of k ascending and k descending, per measure.  The factor covers what the
    stand-in leaves out: the MFMA's unspecified order over its 16 k and the fp32 epilogue (the stand-in's own
    result is rounded to fp32 once, as a stored output is)."""
    model = fn("f64", 1)
    d = [measures(fn("f32", k).astype(np.float32), model) for k in (1, -1)]
    return model, (BAR_FACTOR * max(d[0][0], d[1][0]), BAR_FACTOR * max(d[0][1], d[1][1]))


def nudged_distance(x, layers, taps, nterm, model, seed=0, eps=1e-5):
    """measures() between `model` and the same stack with every hand-over nudged by up to +-2 fp32 ulps"""
    return measures(stack(x, layers, nterm, taps=taps, eps=eps, nudge=np.random.default_rng(seed)), model)


def chain_bar_one_term(x, layers, taps, model, seed=0, eps=1e-5):
    """Fused chains in the one-term mode.  A 1-ulp fp32 difference in a layer's output flips a round-to-nearest hi
    half (2^-11 of the element) for a few elements in ten thousand and no lo term catches it, so the kernel cannot
    be held to the single-layer bar.  The bar is BAR_FACTOR x the relative L2 by which the case's own model moves
    when every hand-over is nudged by up to +-2 fp32 ulps; the worst row is reported, not asserted.
    -> (bar_l2, worst row of the experiment)"""
    l2, row = nudged_distance(x, layers, taps, 1, model, seed, eps)
    return BAR_FACTOR * l2, row


# fp32 partial sums: no thread and no reduction of the kernels adds more than this many terms in a row (a 256 x 256
# tile's half, 32 768 values, over >= 256 threads: 128; resstack64's UpFeed: 4 fragments x 2 blocks x 16 registers x 2:
# 256; then 6 shuffle steps and <= 8 waves)
STATS_CHAIN = 320


def stats_bounds(model, chan_mod, bar_l2):
    """Bounds on |kernel - model| of the four partial sums, from the bar on the outputs and fp32 summation (u =
    2^-24, chains of at most STATS_CHAIN terms): sum of squares 2 bar S2 + chain u S2 (Cauchy-Schwarz on the output
    error); plain sum (bar + chain u) sqrt(n S2), since sum|v| <= sqrt(n) |v|_2.  -> [B][4]"""
    s = stats4(model, chan_mod)
    n = model.shape[1] * model.shape[2] / 2
    u = STATS_CHAIN * 2.0 ** -24
    out = np.empty_like(s)
    for k in (0, 2):
        out[:, k] = (bar_l2 + u) * np.sqrt(n * s[:, k + 1])
        out[:, k + 1] = (2 * bar_l2 + u) * s[:, k + 1]
    return out
