"""CPU-only: the MUSIC / TOPS pruners' host side -- the float64 restatement against the reference's
maps (fixtures g13 / g14), the Prone_method dispatch of MicArray, and the C-ABI argument checks of
the pruner entry points (no GPU call is made)."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

from tests import pruners_restated as pr
from tests.golden.make_golden_pruners import ROI, checksum, scene


@pytest.fixture(scope="module")
def node():
    from acousticswarms_speech_amd.mic_array import MicArray
    mics, _, _ = scene(48000)
    with redirect_stdout(io.StringIO()):
        return MicArray(mics, Spk_Range=ROI).SRP_node


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.mark.parametrize("T,tag", [(48000, "t48"), (144000, "t144")])
def test_restated_music_matches_reference(node, golden, T, tag):
    g = golden("g13_music_map")
    _, _, mix = scene(T)
    np.testing.assert_allclose(checksum(mix), g[f"{tag}_checksum"], rtol=1e-12)
    got = pr.music_map(mix, int(g[f"{tag}_window"]), node)
    assert _rel(g[f"{tag}_map"], got) <= float(g[f"{tag}_spread"]) * (1 + 1e-6)


def test_restated_tops_matches_reference(node, golden):
    g = golden("g14_tops_map")
    _, _, mix = scene(int(g["T"]))
    np.testing.assert_allclose(checksum(mix), g["checksum"], rtol=1e-12)
    got, bins = pr.tops_map(mix, node)
    assert bins.tolist() == g["max_bin"].tolist()
    assert _rel(g["map"], got) <= float(g["spread"]) * (1 + 1e-6)


def test_tops_geometry_tables(node):
    pc = node.grids - node.mic_pos.mean(0)
    mc = node.mic_pos - node.mic_pos.mean(0)
    g, m = 123, 4
    assert node.tops_delta.shape == (node.grids.shape[0], node.num_mic)
    assert np.isclose(node.tops_delta[g, m], np.linalg.norm(pc[g]) - np.linalg.norm(pc[g] - mc[m]), rtol=0, atol=1e-12)
    assert np.isclose(node.tops_coef, 2 * np.pi * node.FS / (node.n_fft * node.C))


@pytest.mark.parametrize("method", ["MUSIC", "TOPS", "SRP"])
def test_mic_array_accepts_pruners(method):
    from acousticswarms_speech_amd.mic_array import MicArray
    mics, _, _ = scene(48000)
    with redirect_stdout(io.StringIO()):
        ma = MicArray(mics, Spk_Range=ROI, Prone_method=method)
    assert ma.Prone_method == method


def test_mic_array_rejects_unknown_pruner():
    from acousticswarms_speech_amd.mic_array import MicArray
    mics, _, _ = scene(48000)
    with pytest.raises(ValueError, match="Prone_method"):
        with redirect_stdout(io.StringIO()):
            MicArray(mics, Spk_Range=ROI, Prone_method="FOO")


def test_apply_dispatches_on_prone_method(golden):
    """Apply_SRP_PHAT calls the map method Prone_method names (the map itself is replaced here)."""
    from acousticswarms_speech_amd.mic_array import MicArray
    g = golden("g13_music_map")
    mics, _, mix = scene(48000)
    with redirect_stdout(io.StringIO()):
        ma = MicArray(mics, Spk_Range=ROI, Prone_method="MUSIC")
    called = []
    node = ma.SRP_node
    node.SRP_Map_WINDOW_new = lambda s, window=36000: called.append("SRP")
    node.MUSIC_Map_WINDOW = lambda s, window=36000: (called.append(("MUSIC", window)), node.set_map(g["t48_map"]))
    with redirect_stdout(io.StringIO()):
        patches, _ = ma.Apply_SRP_PHAT(mix)
    assert called == [("MUSIC", 24000)]
    np.testing.assert_array_equal(np.stack([p.sample_offset for p in patches]), g["t48_offsets"])


def test_pruner_abi_rejects_bad_arguments_without_a_gpu():
    from acousticswarms_speech_amd import native
    L = native.lib()
    assert L.asw_pruner_covariance(None, 7, 48000, 24000, 24000, 2, 2048, 512, 2, 198, None, None, None) == -1
    assert b"pruner_covariance" in L.asw_last_error()
    x = np.zeros(4, dtype=np.float64)
    p = x.ctypes.data
    assert L.asw_pruner_covariance(p, 17, 48000, 24000, 24000, 2, 2048, 512, 2, 198, p, p, None) == -1
    assert L.asw_pruner_covariance(p, 7, 48000, 24000, 24000, 3, 2048, 512, 2, 198, p, p, None) == -1
    assert b"past the signal" in L.asw_last_error()
    assert L.asw_hermitian_eigh(None, 4, 7, None, None, None) == -1
    assert b"hermitian_eigh" in L.asw_last_error()
    assert L.asw_hermitian_eigh(p, 4, 17, p, p, None) == -1
    assert L.asw_music_map(None, 2, 198, 7, None, 100, None, None, None, None, None) == -1
    assert b"music_map" in L.asw_last_error()
    assert L.asw_music_map(p, 2, 198, 3, p, 100, p, p, p, p, None) == -1
    assert L.asw_tops_map(None, None, 2, 198, 2, 7, None, 100, 1.0, None, None, None, None) == -1
    assert b"tops_map" in L.asw_last_error()
    assert L.asw_tops_map(p, p, 2, 1, 2, 7, p, 100, 1.0, p, p, p, None) == -1
