"""The attention kernels (csrc/attention.hip, and the inter-speaker attention of csrc/sep_kernels.hip) on softmax rows
that are not flat: statements, input families, the case table and the bars.  Plain module: no test, no fixture.
tests/test_attention_cases_host.py checks all of it without a GPU, tests/test_gpu_attention_edges.py runs the kernels.

Statements.  attention_f64 / relpos_attention_f64 / inter_attention_f64 are float64 numpy statements of the three
operations (nn.MultiheadAttention's core; RelPosMHAXL's, score[i][j] = scale * ((q_i + u_h) . k_j + (q_i + v_h) .
P_h[(L-1) + j - i]) with explicit indexing; the same core over the speaker axis).  *_f32 is the float32 stand-in: the
same statement with every array and every operation in np.float32, the two products added one k at a time (_mm).  It
models nothing; its distance from the float64 statement sizes the bars, as accumulate(acc="f32") does in
tests/f16_model.py, and like there the larger of k ascending and k descending counts (sizing).  attention_f16_model is
the model of attention_mfma16_kernel: Q -> split_attn(float32(q) * float32(1 / sqrt(128))), K, V -> split_attn,
everything after in float64 (the device's hi | lo split of p * 2^12 is good to 2^-23 of p and needs no model).

Families (make_qkv; u = a random unit vector of head_dim per head, A = amplitude(head_dim) = 30 sqrt(head_dim / 128)):
  flat         N(0, 1)
  peaked       q, k x 3: scores reach about +-30, a handful of keys carry a row
  ramp         k_j += c_j u, c_j = A (2 (j // 64) / (ceil(L / 64) - 1) - 1) (0 at L <= 64); q_i += +-A u (even / odd i):
               even rows raise their maximum at every 64-key tile up to the last, partly filled one, odd rows have it
               in the first and everything after underflows; exp(90) overflows float32 without the maximum subtracted
  neg_offset   k_j += a u, q_i -= a u, a = 48 (head_dim / 128)^(1/4): every score near -200
  pos_offset   k_j += a u, q_i += a u: every score near +200
  rel_ramp+/-  (rel-pos only) the large term comes through the skewed (q + v) . P product alone: bias_v += +-A u_h,
               P_m += c'_m u_h, c' a staircase of one step per 64 rows of P from -A to A plus a slope (make_relpos)
The rel-pos routes use the model's own scale 1 / sqrt(d); every amplitude there is multiplied by nhead^(1/4), so that
the PRODUCT of two of them grows by sqrt(nhead) and the scores reach the ranges of the plain routes.  The inter-speaker
route softmaxes over speakers: the same families with the speaker as the sequence axis and a "tile" of one speaker.
"""
import functools
import math
import zlib

import numpy as np

from tests import f16_model as fm

TILE = 64
NHEAD = 2
FAMILIES = ("flat", "peaked", "ramp", "neg_offset", "pos_offset")
REL_FAMILIES = FAMILIES + ("rel_ramp+", "rel_ramp-")
# rel_ramp: P noise, and the rise of the bd term (score units) that the last, partly filled key tile must still show
REL_P_NOISE = 0.2
REL_LAST_RISE = 3.0


# ------------------------------------------------------------------------------------------------------ statements
def _heads(x, nhead):
    B, L, d = x.shape
    return x.reshape(B, L, nhead, d // nhead).transpose(0, 2, 1, 3)            # [B][H][L][hd]


def _merge(o):
    B, H, L, hd = o.shape
    return o.transpose(0, 2, 1, 3).reshape(B, L, H * hd)


def _mm(a, b, order=1):
    """a [..][M][K] @ b [..][K][N].  float64: numpy's product.  float32, the stand-in: one product and one addition
    per k, each rounded to float32, k ascending (order = 1) or descending (-1) -- the order of a chain, which is how every
    kernel here adds (an fmaf chain over head_dim and over the keys, or the f32 MFMA's two k per step); a BLAS product
    would add 8 or 16 partial sums of a tenth of the length and undersize the bars of the rows that hang on few keys."""
    if a.dtype == np.float64:
        return a @ b
    assert a.dtype == np.float32 and b.dtype == np.float32
    acc = np.zeros(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1]), dtype=np.float32)
    for k in list(range(a.shape[-1]))[::order]:
        acc += a[..., :, k, None] * b[..., k, None, :]
    return acc


def _softmax_pv(s, v, order=1):
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    return _mm(p, v, order)


def _qkv(qkv, nhead, dt):
    x = np.asarray(qkv, dtype=dt)
    d = x.shape[-1] // 3
    return [_heads(x[..., i * d:(i + 1) * d], nhead) for i in range(3)]


def attention_scores(qkv, nhead, dt=np.float64, order=1):
    q, k, _v = _qkv(qkv, nhead, dt)
    return _mm(q, k.swapaxes(-1, -2), order) / np.sqrt(dt(q.shape[-1]))        # [B][H][L][L]


def _attention(qkv, nhead, dt, order=1):
    return _merge(_softmax_pv(attention_scores(qkv, nhead, dt, order), _qkv(qkv, nhead, dt)[2], order))


def attention_f64(qkv, nhead):
    """softmax(Q K^T / sqrt(head_dim)) V of qkv [B][L][3d] (Q | K | V, head h at columns h * head_dim) -> [B][L][d]"""
    return _attention(qkv, nhead, np.float64)


def attention_f32(qkv, nhead, order=1):
    return _attention(qkv, nhead, np.float32, order)


def attention_f16_model(qkv, nhead):
    """attention_f64 of the operands attention_mfma16_kernel multiplies (head_dim 128)"""
    q, k, v = _qkv(qkv, nhead, np.float32)
    assert q.shape[-1] == 128
    q = fm.split_attn(q * np.float32(1.0 / math.sqrt(128.0)))                   # the scale is applied before the split
    return _merge(_softmax_pv(q @ fm.split_attn(k).swapaxes(-1, -2), fm.split_attn(v)))


def relpos_scores(qkv, P, bu, bv, nhead, scale, dt=np.float64, order=1):
    """-> (ac, bd) [B][H][L][L]: scale (q_i + u_h) . k_j and scale (q_i + v_h) . P_h[(L-1) + j - i]"""
    q, k, _v = _qkv(qkv, nhead, dt)
    B, H, L, hd = q.shape
    u, vb = np.asarray(bu, dt).reshape(1, H, 1, hd), np.asarray(bv, dt).reshape(1, H, 1, hd)
    Ph = np.asarray(P, dt).reshape(2 * L - 1, H, hd).transpose(1, 0, 2)        # [H][2L-1][hd]
    sc = dt(scale)
    ac = _mm((q + u) * sc, k.swapaxes(-1, -2), order)
    g = _mm((q + vb) * sc, Ph.swapaxes(-1, -2)[None], order)                   # [B][H][L][2L-1]
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    return ac, g[:, :, i, (L - 1) + j - i]


def _relpos(qkv, P, bu, bv, nhead, scale, dt, order=1):
    ac, bd = relpos_scores(qkv, P, bu, bv, nhead, scale, dt, order)
    return _merge(_softmax_pv(ac + bd, _qkv(qkv, nhead, dt)[2], order))


def relpos_attention_f64(qkv, P, bu, bv, nhead, scale):
    """RelPosMHAXL's core: qkv [B][L][3d], P [2L-1][d], bu / bv [d] (flat, head-major) -> [B][L][d]"""
    return _relpos(qkv, P, bu, bv, nhead, scale, np.float64)


def relpos_attention_f32(qkv, P, bu, bv, nhead, scale, order=1):
    return _relpos(qkv, P, bu, bv, nhead, scale, np.float32, order)


def _groups(qkv, counts):
    """-> [(first sequence, S)] and qkv as [N][L][3d]"""
    x = np.asarray(qkv)
    if counts is None:
        NB, S, L, d3 = x.shape
        return [(n * S, S) for n in range(NB)], x.reshape(NB * S, L, d3)
    out, n0 = [], 0
    for c in counts:
        if int(c) > 0:
            out.append((n0, int(c)))
            n0 += int(c)
    assert n0 == x.shape[0]
    return out, x


def _inter(qkv, nhead, counts, dt, scores=False, order=1):
    groups, x = _groups(qkv, counts)
    res = [] if scores else np.empty(x.shape[:2] + (x.shape[2] // 3,), dtype=dt)
    for n0, S in groups:
        seq = x[n0:n0 + S].transpose(1, 0, 2)                                  # [L][S][3d]: the speakers are the sequence
        if scores:
            res.append(attention_scores(seq, nhead))
        else:
            res[n0:n0 + S] = _attention(seq, nhead, dt, order).transpose(1, 0, 2)
    return res if scores else res.reshape(np.asarray(qkv).shape[:-1] + (res.shape[-1],))


def inter_attention_f64(qkv, nhead, counts=None):
    """At every (group, time step, head) the speakers of the group attend to each other: qkv [NB][S][L][3d] ->
    [NB][S][L][d]; with counts, qkv [N][L][3d] holds counts[g] consecutive sequences per group (zeros left out)"""
    return _inter(qkv, nhead, counts, np.float64)


def inter_attention_f32(qkv, nhead, counts=None, order=1):
    return _inter(qkv, nhead, counts, np.float32, order=order)


# -------------------------------------------------------------------------------------------------------- families
def amplitude(hd):
    return 30.0 * math.sqrt(hd / 128.0)


def offset_amplitude(hd):
    return 48.0 * math.sqrt(hd / 128.0) ** 0.5


def _units(rng, nhead, hd):
    u = rng.standard_normal((nhead, hd))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def make_qkv(family, B, L, nhead, hd, seed, tile=TILE, base=1.0, gain=1.0):
    """float32 qkv [B][L][3d] of one family; `tile`: keys per step of the ramp; `gain`: on every amplitude"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L, 3, nhead, hd)) * base
    u = _units(rng, nhead, hd)
    q, k = x[:, :, 0], x[:, :, 1]                                               # views [B][L][H][hd]
    pos = np.arange(L)
    if family == "peaked":
        q *= 3.0 * gain
        k *= 3.0 * gain
    elif family == "ramp":
        A = amplitude(hd) * gain
        nt = -(-L // tile)
        c = A * (2.0 * (pos // tile) / (nt - 1) - 1.0) if nt > 1 else np.zeros(L)
        k += c[None, :, None, None] * u
        q += np.where(pos % 2 == 0, A, -A)[None, :, None, None] * u
    elif family in ("neg_offset", "pos_offset"):
        a = offset_amplitude(hd) * gain
        k += a * u
        q += (-a if family == "neg_offset" else a) * u
    else:
        assert family == "flat" or family.startswith("rel_ramp"), family
    return x.reshape(B, L, 3 * nhead * hd).astype(np.float32)


def make_relpos(family, B, L, nhead, hd, seed):
    """-> qkv, P, bu, bv, scale.  flat is the input of test_relpos_attention (0.7 N(0, 1); P 0.7, biases 0.3)."""
    d = nhead * hd
    scale = 1.0 / math.sqrt(d)
    gain = nhead ** 0.25
    rel = family.startswith("rel_ramp")
    qkv = make_qkv(family, B, L, nhead, hd, seed, base=0.7 if family == "flat" or rel else 1.0, gain=gain)
    rng = np.random.default_rng(seed + 1)
    P = rng.standard_normal((2 * L - 1, nhead, hd)) * (REL_P_NOISE if rel else 0.7)
    bu, bv = rng.standard_normal((nhead, hd)) * 0.3, rng.standard_normal((nhead, hd)) * 0.3
    if rel:
        # bd ~ scale * (+-A) * c'_m.  c' = the staircase (one step per 64 rows of P, -A .. A) + a slope: two keys of
        # one row that are kn rows of P apart share a stair for all but kn / 64 of the rows, so without the slope the
        # last, partly filled key tile (kn keys) would not raise the maximum; the slope gives it REL_LAST_RISE.
        u = _units(rng, nhead, hd)
        A = amplitude(hd) * gain
        m = np.arange(2 * L - 1)
        nb = -(-(2 * L - 1) // TILE)
        stair = A * (2.0 * (m // TILE) / (nb - 1) - 1.0) if nb > 1 else np.zeros(2 * L - 1)
        kn = L - TILE * (-(-L // TILE) - 1)
        slope = REL_LAST_RISE / kn / (A * scale) if L > TILE else 0.0
        P += (stair + slope * (m - (L - 1)))[:, None, None] * u
        bv += (A if family.endswith("+") else -A) * u
    f = np.float32
    return qkv, P.reshape(2 * L - 1, d).astype(f), bu.reshape(d).astype(f), bv.reshape(d).astype(f), scale


def make_inter(family, counts, L, nhead, hd, seed):
    """qkv [N][L][3d], N = sum(counts): each group its own family instance along the speaker axis"""
    parts = []
    for g, S in enumerate(c for c in counts if c > 0):
        x = make_qkv(family, L, S, nhead, hd, seed + 7 * g, tile=1)              # [L][S][3d]
        parts.append(x.transpose(1, 0, 2))
    return np.ascontiguousarray(np.concatenate(parts, axis=0))


# ---------------------------------------------------------------------------------------------------------- cases
class Case:
    """One launch.  kind: "attn" | "relpos" | "inter"; prefix: what the launch name starts with (relpos_attention_mfma
    also starts with relpos_attention, so the VALU routes name what must NOT follow); child: runs under
    ASW_RELPOS_VALU=1 in a process of its own"""

    def __init__(self, route, kind, prefix, precision, hd, L, family, counts=None, child=False):
        self.route, self.kind, self.prefix, self.precision = route, kind, prefix, precision
        self.hd, self.L, self.family, self.counts, self.child = hd, L, family, counts, child
        self.B, self.nhead, self.d = 2, NHEAD, NHEAD * hd
        shape = f"L{L}" if counts is None else "S" + "_".join(map(str, counts))
        self.id = f"{route}-hd{hd}-{shape}-{family}"
        # the inputs depend on the operation and the shape, not on the route: mfma16 and mfma64 share them
        self.seed = zlib.crc32(f"{kind}-{hd}-{shape}-{family}".encode()) % (1 << 31)

    def name_ok(self, name):
        if not name.startswith(self.prefix):
            return False
        return self.route not in ("relpos_valu", "relpos_valu64") or not name.startswith("relpos_attention_mfma")


ROUTES = (
    # route, kind, launch-name prefix, precision, head dims, lengths, families
    ("mfma16", "attn", "attention_mfma16", "f16x3", (128,), (1, 63, 64, 65, 130, 320), FAMILIES),
    ("mfma64", "attn", "attention_mfma64", "f32", (128,), (1, 63, 64, 65, 130, 320), FAMILIES),
    ("flash", "attn", "attention_mfma_flash", "f32", (128,), (321, 385), FAMILIES),
    ("valu", "attn", "attention_valu", "f32", (16, 48, 112), (1, 15, 16, 17, 128, 129, 260), FAMILIES),
    ("relpos_mfma", "relpos", "relpos_attention_mfma", None, (64,), (1, 63, 64, 65, 130, 200), REL_FAMILIES),
    ("relpos_valu", "relpos", "relpos_attention", None, (16, 32), (1, 16, 17, 64, 65, 130), REL_FAMILIES),
    ("relpos_valu64", "relpos", "relpos_attention", None, (64,), (1, 64, 65, 130), REL_FAMILIES),
)
INTER_S = (1, 2, 27, 64)
INTER_L = 3
INTER_GROUPS = (3, 0, 1, 6, 2)


@functools.lru_cache(maxsize=None)
def all_cases():
    out = {}
    for route, kind, prefix, prec, hds, Ls, fams in ROUTES:
        for hd in hds:
            for L in Ls:
                for fam in fams:
                    c = Case(route, kind, prefix, prec, hd, L, fam, child=route == "relpos_valu64")
                    out[c.id] = c
    for hd in (16, 64):
        for fam in FAMILIES:
            for S in INTER_S:
                c = Case("inter", "inter", "inter_attention", None, hd, INTER_L, fam, counts=(S, S))
                out[c.id] = c
            c = Case("inter_groups", "inter", "inter_attention_groups", None, hd, INTER_L, fam, counts=INTER_GROUPS)
            out[c.id] = c
    return out


def case_ids(child=False):
    return [k for k, c in all_cases().items() if c.child == child]


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """the case's float32 inputs (unchanged by everyone who reads them)"""
    c = all_cases()[cid]
    if c.kind == "attn":
        return (make_qkv(c.family, c.B, c.L, c.nhead, c.hd, c.seed),)
    if c.kind == "relpos":
        return make_relpos(c.family, c.B, c.L, c.nhead, c.hd, c.seed)
    return (make_inter(c.family, c.counts, c.L, c.nhead, c.hd, c.seed),)


def statement(c, dt, order=1):
    inp = inputs(c.id)
    if c.kind == "attn":
        return _attention(inp[0], c.nhead, dt, order)
    if c.kind == "relpos":
        return _relpos(*inp[:4], c.nhead, inp[4], dt, order)
    return _inter(inp[0], c.nhead, c.counts, dt, order=order)


def scores(c):
    """float64 scores: attn -> s; relpos -> (ac + bd, bd); inter -> one array [L][H][S][S] per group"""
    inp = inputs(c.id)
    if c.kind == "attn":
        return attention_scores(inp[0], c.nhead)
    if c.kind == "relpos":
        ac, bd = relpos_scores(*inp[:4], c.nhead, inp[4])
        return ac + bd, bd
    return _inter(inp[0], c.nhead, c.counts, np.float64, scores=True)


def rows(c, out):
    """output -> rows of head_dim values, one per (item, position, head): what measures() pools"""
    out = np.asarray(out)
    return out.reshape(-1, c.hd)


@functools.lru_cache(maxsize=None)
def sizing(cid):
    """-> dict: truth (the float64 statement), model (what the kernel is compared with: the truth, or on the f16 route
    the split-operand model), model_vs_truth, bar_l2, bar_row = BAR_FACTOR x the distance between the float64 statement
    and its float32 stand-in, per measure"""
    c = all_cases()[cid]
    truth = statement(c, np.float64)
    d = [0.0, 0.0]
    for order in (1, -1):                                   # as f16_model.bars: the larger of k ascending and descending
        standin = statement(c, np.float32, order)
        assert standin.dtype == np.float32
        d = [max(a, b) for a, b in zip(d, fm.measures(rows(c, standin), rows(c, truth)))]
    model = attention_f16_model(inputs(cid)[0], c.nhead) if c.precision == "f16x3" else truth
    return dict(truth=truth, model=model, model_vs_truth=fm.measures(rows(c, model), rows(c, truth)),
                bar_l2=fm.BAR_FACTOR * d[0], bar_row=fm.BAR_FACTOR * d[1])


# ------------------------------------------------------------------------------------------------------ conditions
def tile_steps(s, tile=TILE):
    """scores [..][L][L] -> (fraction of even rows whose tile maxima rise by >= 1 at every step, fraction of odd rows
    whose tile maxima fall by >= 1 at every step, fraction of ALL rows that rise, of all rows that fall)"""
    L = s.shape[-1]
    nt = -(-L // tile)
    tm = np.stack([s[..., t * tile:(t + 1) * tile].max(-1) for t in range(nt)], axis=-1)      # [..][L][nt]
    df = np.diff(tm, axis=-1)
    up, down = np.all(df >= 1.0, axis=-1), np.all(df <= -1.0, axis=-1)
    even = np.arange(L) % 2 == 0
    return float(up[..., even].mean()), float(down[..., ~even].mean()), float(up.mean()), float(down.mean())


def participation(s):
    """median over rows of 1 / sum(p^2)"""
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    return float(np.median(1.0 / (p ** 2).sum(-1)))


def conditions(c):
    """the figures the host test asserts on: dict with lo, hi (score range), part (participation), and for the ramps
    even_up / odd_down / all_up / all_down (the full score), bd_up / bd_down (rel_ramp: the bd term alone)"""
    s = scores(c)
    out = {}
    if c.kind == "inter":
        out["lo"], out["hi"] = min(float(g.min()) for g in s), max(float(g.max()) for g in s)
        out["part"] = float(np.median([participation(g) for g in s]))
        return out
    full, bd = s if c.kind == "relpos" else (s, None)
    out["lo"], out["hi"], out["part"] = float(full.min()), float(full.max()), participation(full)
    if c.L > TILE:
        out["even_up"], out["odd_down"], out["all_up"], out["all_down"] = tile_steps(full)
        if bd is not None:
            _e, _o, out["bd_up"], out["bd_down"] = tile_steps(bd)
    return out
