"""Full BSS-eval (SDR, SIR, SAR, best permutation), the parts that need no GPU: the host statement against
``bss_eval_sdr`` and its own identities, the conditioning of the inputs the GPU tests use, ``best_permutation``, the
workspace formula and the packing rule in both modes, the refusals of the C entry point (all before the first launch),
the Python layer's errors, the route back to the host for items the device marks, and the records."""
import ctypes
import functools
import itertools
import re

import numpy as np
import pytest
import torch

from acousticswarms_speech_amd import evalkit, native

from tests import bss_eval_cases as cases
from tests import bss_sources_cases as sc
from tests.bss_sources_cases import c_bytes as _c_bytes, stand_in as _stand_in

SMALL = [c for c in sc.MATCHED if c not in sc.WORKING]


# ---- the statement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.RAGGED[:4] + sc.LENGTHS[:1], ids=str)
def test_matched_statement_is_bss_eval_sdr_byte_for_byte(case):
    seed, counts, T, flen, kinds = case
    refs, ests, want = sc.matched(*case)
    n0 = 0
    for ref, est in zip(refs, ests):
        S = ref.shape[0]
        for r in range(len(kinds) if S else 0):
            sdr, sir, sar, perm = evalkit.bss_eval_sources(ref, est[r], flen)
            assert sdr.tobytes() == evalkit.bss_eval_sdr(ref, est[r], flen).tobytes()
            assert sdr.tobytes() == want[0, r, n0:n0 + S].tobytes()
            assert perm.tolist() == list(range(S))
            m = evalkit.bss_eval_matrices(ref, est[r], flen)              # the diagonal of the matrix form is the vector form
            for vec, mat in zip((sdr, sir, sar), m):
                assert np.diag(mat).tobytes() == vec.tobytes()
        n0 += S


def _all_statement_values():
    """(tag, sdr, sir, sar) of every input the GPU tests use."""
    for case in sc.MATCHED:
        yield ("matched", case), *sc.matched(*case)[2]
    for case in sc.PAIRS:
        yield ("pairs", case), *sc.pairs(*case)[2]
    for case in sc.SHUFFLED:
        for k, m in enumerate(sc.shuffled(*case)[3]):
            yield ("shuffled", case, k), m[:, 0], m[:, 1], m[:, 2]


def test_identities_and_conditioning_of_the_device_test_inputs():
    """sdr <= min(sir, sar) (the SDR's distortion is both others' and more); one talker has sir == +inf; every finite SIR
    and SAR of the inputs the device is compared on lies in -30 .. +50 dB, where the differences of nearly equal
    projections they are made of still carry digits."""
    lo = {"sir": np.inf, "sar": np.inf}
    hi = {"sir": -np.inf, "sar": -np.inf}
    for tag, sdr, sir, sar in _all_statement_values():
        assert np.all(sdr <= np.minimum(sir, sar) + 1e-9), tag
        assert not np.any(np.isnan(sir)) and np.all(np.isfinite(sar)) and np.all(np.isfinite(sdr)), tag
        for name, v in (("sir", sir), ("sar", sar)):
            f = v[np.isfinite(v)]
            if f.size:
                lo[name], hi[name] = min(lo[name], float(f.min())), max(hi[name], float(f.max()))
            assert np.all((f >= -30.0) & (f <= 50.0)), (tag, name, f.min(), f.max())
    print(f"SIR {lo['sir']:.1f} .. {hi['sir']:.1f} dB, SAR {lo['sar']:.1f} .. {hi['sar']:.1f} dB")
    for case in sc.MATCHED:
        counts, want = case[1], sc.matched(*case)[2]
        n0 = 0
        for S in counts:
            assert np.all(np.isinf(want[1, :, n0:n0 + S]) == (S == 1)), case
            n0 += S


def test_one_talker_has_infinite_sir():
    rng = np.random.default_rng(3)
    ref = cases.references(rng, 1, 500)
    sdr, sir, sar, perm = evalkit.bss_eval_sources(ref, cases.estimates(rng, ref, "noisy"), 8, compute_permutation=True)
    assert sir.tolist() == [np.inf] and perm.tolist() == [0] and np.isfinite(sdr[0]) and sdr[0] == sar[0]


def test_shape_errors_of_the_statement():
    with pytest.raises(ValueError, match="shapes differ"):
        evalkit.bss_eval_sources(np.zeros((2, 100)), np.zeros((3, 100)), 8)
    with pytest.raises(ValueError, match="shapes differ"):
        evalkit.bss_eval_matrices(np.zeros((2, 100)), np.zeros((2, 99)), 8)
    with pytest.raises(ValueError, match="not square"):
        evalkit.best_permutation(np.zeros((2, 3)))


# ---- the permutation --------------------------------------------------------------------------------------------------
def _means(sir):
    S = sir.shape[0]
    return sorted((float(np.mean(sir[list(p), np.arange(S)])) for p in itertools.permutations(range(S))), reverse=True)


@pytest.mark.parametrize("case", sc.SHUFFLED, ids=str)
def test_statement_recovers_a_known_shuffle_with_a_margin(case):
    refs, ests, perms, mats = sc.shuffled(*case)
    flen = case[3]
    for ref, est, perm, m in zip(refs, ests, perms, mats):
        for r in range(2):
            sdr, sir, sar, got = evalkit.bss_eval_sources(ref, est[r], flen, compute_permutation=True)
            assert got.tolist() == perm[r].tolist()
            idx = np.arange(ref.shape[0])
            for vec, q in zip((sdr, sir, sar), range(3)):
                assert vec.tobytes() == m[r, q][perm[r], idx].tobytes()
            if ref.shape[0] > 1:
                best, second = _means(m[r, 1])[:2]
                print(f"{case} set {r}: best mean SIR {best:.2f} dB, second {second:.2f} dB")
                assert best - second >= 1.0
            # put back in order, the vectors are those of the matched statement on the unshuffled rows
            back = evalkit.bss_eval_sources(ref, est[r][perm[r]], flen)
            assert back[1].tobytes() == sir.tobytes() and back[2].tobytes() == sar.tobytes()


def test_best_permutation_by_hand():
    bp = evalkit.best_permutation
    assert bp(np.zeros((0, 0))).tolist() == [] and bp(np.array([[3.0]])).tolist() == [0]
    assert bp(np.array([[np.inf]])).tolist() == [0]
    # perm[j] = the estimate (row) of reference (column) j
    assert bp(np.array([[1.0, 9.0], [8.0, 2.0]])).tolist() == [1, 0]
    assert bp(np.array([[9.0, 1.0], [2.0, 8.0]])).tolist() == [0, 1]
    m = np.array([[0.0, 5.0, 1.0], [1.0, 0.0, 7.0], [6.0, 2.0, 0.0]])          # est 2 -> ref 0, est 0 -> ref 1, est 1 -> ref 2
    assert bp(m).tolist() == [2, 0, 1]
    # the mean decides, not the best single entry: 10 + 0 < 6 + 6
    assert bp(np.array([[10.0, 6.0], [6.0, 0.0]])).tolist() == [1, 0]
    # a tie goes to the first permutation in itertools order
    assert bp(np.zeros((3, 3))).tolist() == [0, 1, 2]
    # a +inf entry: every permutation through it has mean +inf, the first of them in order wins
    m = np.array([[1.0, np.inf, 0.0], [5.0, 0.0, 2.0], [0.0, 3.0, 9.0]])
    assert bp(m).tolist() == [1, 0, 2]
    # above 6 talkers the assignment takes a +inf entry too, and the best of the rest
    big = np.arange(64, dtype=np.float64).reshape(8, 8) % 7
    big[3, 5] = np.inf
    perm = bp(big)
    assert sorted(perm.tolist()) == list(range(8)) and perm[5] == 3
    rest = [j for j in range(8) if j != 5]
    sub = big[np.ix_([e for e in range(8) if e != 3], rest)]
    assert np.isclose(sum(big[perm[j], j] for j in rest), max(_means(sub)) * 7)


def test_enumeration_equals_assignment_up_to_six():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(6)
    for S in range(1, 7):
        for _ in range(20):
            sir = rng.normal(10.0, 12.0, (S, S))                               # continuous: no ties
            est_of, ref_of = linear_sum_assignment(sir, maximize=True)
            want = np.zeros(S, dtype=np.int64)
            want[ref_of] = est_of
            assert evalkit.best_permutation(sir).tolist() == want.tolist()
    # and the route above six, against enumeration written out here
    for _ in range(3):
        sir = rng.normal(10.0, 12.0, (7, 7))
        best = max(itertools.permutations(range(7)), key=lambda p: np.mean(sir[list(p), np.arange(7)]))
        assert evalkit.best_permutation(sir).tolist() == list(best)


# ---- workspace and packing ----------------------------------------------------------------------------------------------
def test_workspace_formula_equals_the_library():
    rng = np.random.default_rng(41)
    shapes = [([5], 2, 48000, 512), ([2], 2, 16000, 512), ([1], 1, 64, 64), ([0, 2, 0], 2, 257, 21), ([3, 1, 2], 3, 4099, 43),
              ([], 2, 100, 10), ([0], 1, 100, 10), ([1, 1, 0, 1], 2, 300, 7), ([16], 2, 9000, 512)]
    for _ in range(40):
        flen = int(rng.integers(1, 200))
        shapes.append(([int(c) for c in rng.integers(0, 9, rng.integers(1, 6))], int(rng.integers(1, 4)),
                       int(flen + rng.integers(0, 5000)), flen))
    for counts, R, T, flen in shapes:
        for all_pairs in (False, True):
            got = evalkit.bss_sources_workspace_bytes(counts, R, T, flen, all_pairs)
            assert got == _c_bytes(counts, R, T, flen, all_pairs), (counts, R, T, flen, all_pairs)
            assert evalkit.bss_sources_workspace_bytes(counts, R, T, flen, all_pairs, sdr_only=True) <= got
        # matched and SDR only: the size of the SDR entry, by its formula and by the library
        only = evalkit.bss_sources_workspace_bytes(counts, R, T, flen, False, sdr_only=True)
        assert only == evalkit.bss_workspace_bytes(counts, R, T, flen) == _c_bytes(counts, R, T, flen)
        if all(S <= 1 for S in counts):                                        # one talker: all pairs is the one pair
            assert evalkit.bss_sources_workspace_bytes(counts, R, T, flen, True) == \
                evalkit.bss_sources_workspace_bytes(counts, R, T, flen, False)
    # all pairs at 5 talkers adds 5 * 4 * 2 single solutions of 512 and as many rows of partials, not a system
    extra = evalkit.bss_sources_workspace_bytes([5], 2, 48000, 512, True) - evalkit.bss_sources_workspace_bytes([5], 2, 48000, 512)
    assert 0 < extra < 1 << 20


def test_packing_default_is_todays_and_all_pairs_keeps_the_properties():
    rng = np.random.default_rng(20261020)
    for _ in range(200):
        K = int(rng.integers(0, 12))
        counts = [int(c) for c in rng.integers(0, 5, K)]
        lengths = [int(t) for t in rng.choice([600, 700], K, p=[0.8, 0.2])]
        R, flen = int(rng.integers(1, 3)), int(rng.integers(1, 65))

        def size(c, t):
            return evalkit.bss_sources_workspace_bytes(c, R, t, flen, True)
        alone = max([size([c], t) for c, t in zip(counts, lengths)] + [1])
        budget = int(alone * rng.uniform(1.0, 4.0))
        calls = evalkit.pack_bss_items(counts, lengths, R, flen, budget, all_pairs=True, sdr_only=False)
        assert [k for a, b in calls for k in range(a, b)] == list(range(K))       # whole, in order, once
        for a, b in calls:
            assert b > a and len(set(lengths[a:b])) == 1
            assert size(counts[a:b], lengths[a]) <= budget
        for (a, b), (c, d) in zip(calls, calls[1:]):                               # greedy: the next item did not fit
            assert lengths[c] != lengths[a] or size(counts[a:c + 1], lengths[a]) > budget
        assert evalkit.pack_bss_items(counts, lengths, R, flen, budget, all_pairs=True, sdr_only=False) == calls
        # the default arguments size the calls as bss_workspace_bytes does
        alone = max([evalkit.bss_workspace_bytes([c], R, t, flen) for c, t in zip(counts, lengths)] + [1])
        budget = int(alone * rng.uniform(1.0, 4.0))
        calls = evalkit.pack_bss_items(counts, lengths, R, flen, budget)
        assert calls == evalkit.pack_bss_items(counts, lengths, R, flen, budget, all_pairs=False)
        for a, b in calls:
            assert evalkit.bss_workspace_bytes(counts[a:b], R, lengths[a], flen) <= budget
        for (a, b), (c, d) in zip(calls, calls[1:]):
            assert lengths[c] != lengths[a] or evalkit.bss_workspace_bytes(counts[a:c + 1], R, lengths[a], flen) > budget
    with pytest.raises(RuntimeError, match="alone needs"):
        evalkit.pack_bss_items([3], [1000], 2, 64, budget=evalkit.bss_sources_workspace_bytes([3], 2, 1000, 64, True) - 1,
                               all_pairs=True, sdr_only=False)


# ---- the C entry point refuses on the host, before the first launch: host memory stands in for every pointer ---------
_call = functools.partial(sc.c_call, "asw_bss_eval_sources")


@pytest.mark.parametrize("all_pairs", [0, 1])
@pytest.mark.parametrize("kw,message", [
    (dict(null=("ref",)), "null pointer"), (dict(null=("est",)), "null pointer"), (dict(null=("sdr",)), "null pointer"),
    (dict(null=("ws",)), "null pointer"), (dict(null=("status",)), "null status"), (dict(null=("counts",)), "null counts"),
    (dict(null=("sir",)), "sir and sar go together"), (dict(null=("sar",)), "sir and sar go together"),
    (dict(K=-1), "K = -1 < 0"), (dict(R=0), "R = 0 < 1"),
    (dict(flen=0), "flen = 0 outside"), (dict(flen=1025, T=2000, counts=(1,)), "flen = 1025 outside"),
    (dict(T=7), "T = 7 outside flen = 8"),
    (dict(counts=(2, -1)), r"counts\[1\] = -1 outside 0..16"), (dict(counts=(17,)), r"counts\[0\] = 17 outside 0..16"),
    (dict(counts=(1, 9), flen=1000, T=1000), "item 1: 9 references of 1000 taps make a system of order 9000 > 8192"),
    (dict(ws_delta=-1), "too small"), (dict(ws_shift=4), "not 8-byte aligned"),
    (dict(null=("sir", "sar"), sdr_only_size=True, ws_delta=-1), "too small"),
])
def test_c_refusals(kw, message, all_pairs):
    rc, msg, need = _call(all_pairs=all_pairs, **kw)
    assert rc == -1
    assert msg.startswith("bss_eval_sources: ") and re.search(message, msg), msg


def test_c_refuses_another_mode_and_the_query_refuses_like_the_call():
    rc, msg, _need = _call(all_pairs=2)
    assert rc == -1 and "all_pairs = 2 is neither 0 nor 1" in msg
    L = native.lib()
    c = (ctypes.c_int32 * 2)(2, 17)
    assert L.asw_bss_eval_sources_workspace_bytes(c, 2, 2, 100, 8, 1) == 0
    assert "counts[1] = 17" in L.asw_last_error().decode()
    assert L.asw_bss_eval_sources_workspace_bytes(c, 1, 2, 100, 8, 2) == 0
    assert "all_pairs = 2" in L.asw_last_error().decode()
    assert L.asw_bss_eval_sources_workspace_bytes(c, 1, 2, 100, 8, 1) > L.asw_bss_eval_sources_workspace_bytes(c, 1, 2, 100, 8, 0) > \
        L.asw_bss_eval_sdr_workspace_bytes(c, 1, 2, 100, 8) > 0


def test_c_empty_batch_launches_nothing():
    for all_pairs in (0, 1):
        rc, _msg, need = _call(counts=(), K=0, all_pairs=all_pairs)
        assert rc == 0 and need == 0
        assert native.lib().asw_bss_eval_sources(None, None, None, 0, 1, 10, 5, all_pairs, None, None, None, None, None, 0,
                                                 None) == 0


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def _want(refs, ests, flen, permute):
    out = []
    for r, e in zip(refs, ests):
        sets = [evalkit.bss_eval_sources(r, e[s], flen, permute) for s in range(e.shape[0])]
        out.append(tuple(np.stack([s[q] for s in sets]).reshape(e.shape[0], r.shape[0]) for q in range(4)))
    return out


@pytest.mark.parametrize("permute", [False, True])
def test_marked_items_are_recomputed_on_the_host(permute):
    refs, ests, _perms, _m = sc.shuffled(31, (2, 1, 0, 3), 400, 16)
    want = _want(refs, ests, 16, permute)
    seen = []
    got, redone = evalkit.bss_eval_sources_batch(refs, ests, flen=16, compute_permutation=permute, op=_stand_in({1, 3}, seen))
    assert redone == [1, 3] and len(seen) == 1
    assert seen[0] == ((6, 400), (2, 6, 400), [2, 1, 0, 3], 16, permute)
    for g, w in zip(got, want):
        assert len(g) == 4
        for a, b in zip(g, w):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()
        assert g[0].dtype == np.float64 and g[3].dtype == np.int64
    # several calls: the marks are per call, the reported items per batch
    seen = []
    budget = evalkit.bss_sources_workspace_bytes([2, 1, 0, 3], 2, 400, 16, permute) - 1
    got, redone = evalkit.bss_eval_sources_batch(refs, ests, flen=16, compute_permutation=permute, op=_stand_in({0}, seen),
                                                 budget=budget)
    assert [s[2] for s in seen] == [[2, 1, 0], [3]] and redone == [0, 3]
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.tobytes() == b.tobytes()
    one = evalkit.bss_eval_sources_device(refs[3], ests[3], flen=16, compute_permutation=permute, op=_stand_in(set(), []))
    for a, b in zip(one, want[3]):
        assert a.tobytes() == b.tobytes()
    assert evalkit.bss_eval_sources_batch([], []) == ([], [])


def test_batch_errors_and_missing_gpu(monkeypatch):
    refs, ests = cases.make_batch(5, [2, 1], 400)
    op = _stand_in(set(), [])
    with pytest.raises(ValueError, match="estimate sets for"):
        evalkit.bss_eval_sources_batch(refs, ests[:1], op=op)
    with pytest.raises(ValueError, match="do not go with"):
        evalkit.bss_eval_sources_batch(refs, [ests[0], ests[1][:1]], flen=16, op=op)
    with pytest.raises(ValueError, match="do not go with"):
        evalkit.bss_eval_sources_batch(refs, [ests[0][0], ests[1][0]], flen=16, op=op)
    with pytest.raises(ValueError, match="fewer than flen"):
        evalkit.bss_eval_sources_batch(refs, ests, flen=512, op=op)
    with pytest.raises(RuntimeError, match="alone needs"):
        evalkit.bss_eval_sources_batch(refs, ests, flen=16, op=op, budget=1000)
    ref = np.ones((1, 600))
    for fn, args in ((evalkit.compute_metrics, (ref, ref, ref)), (evalkit.evaluate_sample, (None, {}, ref, ref)),
                     (evalkit.evaluate_dataset, (None, "/nonexistent")), (evalkit.records_from_results, ([], [])),
                     (evalkit.record_from_result, ({}, ref, ref, {}))):
        with pytest.raises(ValueError, match="bss must be one of"):
            fn(*args, bss="sir")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        evalkit.bss_eval_sources_device(ref, ref[None], flen=8)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        evalkit.compute_metrics(ref, ref, ref, metrics="device", bss="all")
    monkeypatch.setattr(native, "_ops", None)
    monkeypatch.setattr(native, "OPS_PATH", "/nonexistent/libasw_torch_ops.so")
    with pytest.raises(RuntimeError, match="is missing"):
        evalkit.bss_eval_sources_device(ref, ref[None], flen=8)


def test_command_line_option():
    from acousticswarms_speech_amd.evaluate import build_parser
    assert build_parser().parse_args(["d"]).bss == "sdr"
    assert build_parser().parse_args(["d", "--bss", "all"]).bss == "all"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["d", "--bss", "sir"])


# ---- records --------------------------------------------------------------------------------------------------------------
EXTRA = ("sir_in_mir", "sir_mir", "sar_in_mir", "sar_mir")


def _sample(S, T=2400, seed=8):
    """A sample and a search result that finds every talker at its place: estimates "noisy", mixture = sum."""
    rng = np.random.default_rng([seed, S])
    gt = cases.references(rng, S, T)
    est = cases.estimates(rng, gt, "noisy")
    mics = np.array([[0.05 * np.cos(a), 0.05 * np.sin(a), 0.0] for a in np.arange(4) * np.pi / 2])
    pos = np.array([[1.0 + 0.8 * s, 0.5 - 0.7 * s, 0.0] for s in range(S)])
    meta = {"ROI": [-3, 3, -3, 3, 0, 0.1]}
    for m in range(4):
        meta[f"mic{m:02d}"] = {"position": mics[m].tolist()}
    for s in range(S):
        meta[f"voice{s:02d}"] = {"position": pos[s].tolist()}
    mix = np.repeat(gt.sum(axis=0, keepdims=True), 4, axis=0).astype(np.float32)
    result = {"centres": pos + 0.01, "offsets": [np.zeros(3) for _ in range(S)], "audio_offsets": [np.zeros(3) for _ in range(S)],
              "audio_loc": est, "audio": None}
    return (meta, mix, gt), result


@pytest.mark.parametrize("S", [1, 2])
def test_records_sdr_untouched_and_all_adds_four_fields(S):
    sample, result = _sample(S)
    plain, *counts = evalkit.record_from_result(*sample, result)
    same, *counts_s = evalkit.record_from_result(*sample, result, bss="sdr")
    full, *counts_a = evalkit.record_from_result(*sample, result, bss="all")
    assert counts == counts_s == counts_a == [S, 0, 0]
    import json
    assert json.dumps(plain) == json.dumps(same)
    assert len(full["pred"]) == S
    for p, f in zip(plain["pred"], full["pred"]):
        assert list(f)[:len(p)] == list(p) and tuple(list(f)[len(p):]) == EXTRA
        assert all(f[k] == p[k] for k in p)
    meta, mix, gt = sample
    pa = np.array(full["perm"])
    inp = np.repeat(mix[0:1].astype(np.float64), S, axis=0)
    s_in, s_out = evalkit.bss_eval_sources(gt[pa[:, 1]], inp), evalkit.bss_eval_sources(gt[pa[:, 1]], result["audio_loc"][pa[:, 0]])
    for i, f in enumerate(full["pred"]):
        assert (f["sir_in_mir"], f["sir_mir"], f["sar_in_mir"], f["sar_mir"]) == (s_in[1][i], s_out[1][i], s_in[2][i], s_out[2][i])
        assert not any(np.isnan(f[k]) for k in EXTRA) and (f["sir_mir"] == np.inf) == (S == 1)
    # the batch form on the host is the per-sample form
    both = evalkit.records_from_results([sample], [result], bss="all")
    assert json.dumps(both[0][0]) == json.dumps(full)


def test_batched_device_records_go_out_in_one_call_of_the_stand_in():
    """``metrics="device"`` with stand-ins for both ops: the whole group goes out in ONE ``bss_eval_sources`` call (matched
    mode), and the records equal the host's in every field, since both stand-ins ARE the host statements."""
    import json
    samples, results = zip(*[_sample(S, seed=9 + S) for S in (2, 1, 3)])
    seen = []

    def cross(est, ref, est_counts, ref_counts):
        out, e0, r0 = [], 0, 0
        for P, S in zip(est_counts, ref_counts):
            out.append(evalkit.cross_sisdr_f64(est[e0:e0 + P].numpy(), ref[r0:r0 + S].numpy()).reshape(-1))
            e0, r0 = e0 + P, r0 + S
        return torch.from_numpy(np.concatenate(out)), torch.zeros(len(est_counts), dtype=torch.int32)
    host = evalkit.records_from_results(list(samples), list(results), bss="all")
    dev = evalkit.records_from_results(list(samples), list(results), metrics="device", ops=(cross, _stand_in(set(), seen)), bss="all")
    assert len(seen) == 1 and seen[0][2] == [2, 1, 3] and seen[0][4] is False
    assert json.dumps(host) == json.dumps(dev)
    sdr_only = evalkit.records_from_results(list(samples), list(results), bss="sdr")
    for (h, *_), (s, *_) in zip(host, sdr_only):
        for ph, ps in zip(h["pred"], s["pred"]):
            assert {k: v for k, v in ph.items() if k not in EXTRA} == ps
