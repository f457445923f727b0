"""Search orchestration of localization-by-separation (SURVEY.md §8 a-M): the four stage
methods of the reference ``Mic_Array`` (sep/Mic_Array.py:95-500) with the same names,
arguments and return layouts.  The per-candidate arithmetic (shift, spot network,
energies) is behind ``spot_model`` on the GPU; SRP-PHAT behind ``SRPPhat``; what remains
here is list bookkeeping, thresholds and the greedy SI-SDR clustering, which follow the
reference including its order-dependent quirks (documented inline).
"""
import numpy as np

from .dense_grid import LatticePatches, lattice_patches
from .fine_cluster import clusters_of_group
from .global_cluster import clusters_of_labels
from .hostdsp import mean_removed_energies, si_sdr, split_wav, split_wise_sisdr
from .modes import LATTICE_METHODS, MODE_NAMES, check_modes, need_methods
from .native import read_back
from .patch import FS, SPEED_OF_SOUND, Patch, pair_offsets
from . import search
from .search import (INIT_WIDTH, SPOT_POWER_THRESHOLD2, USE_RELATIVE_SPOT_POWER, binary_search_baseline,
                     search_area)
from .srp import SRPPhat

FINE_CHUNK_EDGES = (0.0, 0.07, 0.40, 0.73, 0.93, 1.0)      # pipelined fine stage, see _fine_stage_pipelined

# sep/helpers/constants.py:24-27
BIN0, BIN1, N_FFT = 2, 200, 2048
FREQ_BINS = np.arange(BIN0, BIN1)

# pruning map of stage 1 per Prone_method (sep/Mic_Array.py:165-170).  "DENSE" has none: stage 1 is then the whole
# coarse TDoA lattice of the array (dense_grid.coarse_lattice), built once with the geometry.  "DENSE_NMS" is "DENSE"
# with a coarse stage that keeps only the lattice's local maxima (dense_grid.lattice_local_maxima)
PRONE_METHODS = {"SRP": "SRP_Map_WINDOW_new", "MUSIC": "MUSIC_Map_WINDOW", "TOPS": "TOPS_Map_WINDOW", "DENSE": None,
                 "DENSE_NMS": None}


def check_sisnr_win(sisnr_list, SISNR_THRESHOLD=-2, SISNR_THRESHOLD2=-7):
    """Same talker if some segment is similar (> thr) and none is very different (< thr2)
    (sep/Mic_Array.py:18-28)."""
    v = np.asarray(list(sisnr_list), dtype=np.float64)
    return bool(np.any(v > SISNR_THRESHOLD) and not np.any(v < SISNR_THRESHOLD2))


def weight_mean_pos(patch_list, powers, id_lists):
    """Power-weighted mean position / offsets over the cluster members within 75 % of the
    head's power (sep/Mic_Array.py:32-47)."""
    head = powers[id_lists[0]]
    pos = np.zeros((3,))
    offs = np.zeros(patch_list[0].sample_offset.shape)
    tot = 0
    for i in id_lists:
        if powers[i] < head * 0.75:
            continue
        pos += powers[i] * patch_list[i].center_pos()
        offs += powers[i] * patch_list[i].sample_offset
        tot += powers[i]
    return pos / tot, offs / tot


def find_merge_center(merged_offests, init_area, mic_positions, Big_patch_center, init_samples=None):
    """Patch of width 3 around the merged offsets holding the coarse patch's points that fall
    inside; falls back to the coarse centre (sep/Mic_Array.py:50-81).  The reference's
    widening loop leaves after its first pass (factor 0), which repeats the width-3 test.
    ``init_samples`` may carry pair_offsets(init_area, mic_positions) when the caller tests many
    cluster heads against the same coarse patch (same values, computed once)."""
    P = mic_positions.shape[0] - 1
    patch = Patch(merged_offests, [3 for _ in range(P)], None)
    if init_samples is None:
        init_samples = pair_offsets(init_area, mic_positions, SPEED_OF_SOUND, FS)
    inside = patch.hyperbola_sample(init_samples) == 1
    if np.sum(inside) == 0:
        patch.width_list = [3 for _ in range(P)]
        inside = patch.hyperbola_sample(init_samples) == 1
        if np.sum(inside) > 0:
            patch.area_points = init_area[:, inside]
        else:
            patch.peak_pos = Big_patch_center
    else:
        patch.area_points = init_area[:, inside]
    return patch


# the four stages as the "No spk picked in ..." lines of the reference name them (JointModel/network.py:151-199)
SEARCH_STAGES = ("SRP-PHAT", "Spotform_Big_Patch", "Spotform_Small_Patch", "Clustering")


def run_search(mic_array, spot_model, timed, mix_data, stage_mix=None, srp_stage=None):
    """The four search stages on one mixture -- SRP-PHAT, coarse, fine, clustering -- with the reference's empty-result
    early returns (:151-199), written once: ``JointModel.localize_by_separation`` and the searches of a batch
    (``batching.search_one``) are this with their own timer and their own mixtures.
    ``timed(slot, fn, *args)`` runs a stage and keeps its time in ``slot`` 0..3.  Stage 0 is
    ``srp_stage(mix_data)`` (default: the array's ``Apply_SRP_PHAT``); the scoring stages read ``stage_mix()``, asked
    for after stage 0 has run (default: ``mix_data``).
    -> (final patches, their audio, spot_times, empty): ``empty`` is None after a full run, else the entry of
    ``SEARCH_STAGES`` that came back with nothing, and the first three are then ``[], [], 0``."""
    def nothing(stage):
        return [], [], 0, SEARCH_STAGES[stage]
    patch_list, _ = timed(0, srp_stage or mic_array.Apply_SRP_PHAT, mix_data)
    if stage_mix is not None:
        mix_data = stage_mix()
    if len(patch_list) <= 0:
        return nothing(0)
    patch_list = timed(1, mic_array.Spotform_Big_Patch, mix_data, patch_list, spot_model)
    if len(patch_list) <= 0:
        return nothing(1)
    output_pair = timed(2, mic_array.Spotform_Small_Patch_Parallel, mix_data, patch_list, spot_model)
    if len(output_pair) <= 0:
        return nothing(2)
    audio_final, patch_final, spot_times, _ = timed(3, mic_array.Clustering_new, output_pair)
    if len(patch_final) <= 0:
        return nothing(3)
    return patch_final, audio_final, spot_times, None


class MicArray(object):
    # the modes (modes.MODE_NAMES; ``geometry`` is the SRP node's) of an array whose __init__ did not run
    segments = clustering = global_clustering = coarse = "host"

    def __init__(self, mic_positions, demo=False, Spk_Range=None, grid_size=0.05, Prone_method="SRP",
                 MIN_TRIGGER_POWER=0.5, SRP_fast=False, cached=False, cached_folder=None, device=None,
                 geometry="host", segments="host", clustering="host", global_clustering="host", coarse="host"):
        """The five modes (``modes.MODE_NAMES``), each "host" or "device", are described here and nowhere else.
        ``geometry``: where the SRP stage's geometry tables are built -- "host" (numpy) or "device"
        (csrc/geometry_kernels.hip; same tables, for arrays that change from mixture to mixture).
        ``Prone_method="DENSE"`` takes the pruner out: ``Apply_SRP_PHAT`` returns every width-``INIT_WIDTH`` cube of
        the array's TDoA lattice, and the later stages run on that list unchanged.  ``"DENSE_NMS"`` has the same
        stage 1; its coarse stage keeps a cube only if no cube within ``search.LATTICE_NMS_RADIUS`` cells on every
        pair scored higher, and ``lattice_nms`` = {"radius", "best", "degree"} records the latest search.
        ``segments``: where the global clustering finds the voiced segments of the cluster heads -- "host"
        (``hostdsp.split_wav`` per head) or "device" (one ``voiced_segments`` call of the scorer for all heads, the
        tables handed to its ``segment_sisdr_device`` where they are; needs the HIP spot model).
        ``clustering``: where the fine stage clusters the candidates of its coarse patches -- "host" (per patch:
        sort, thresholds, the greedy SI-SDR loop on one ``pair_sisdr`` read-back, one copy of the heads) or "device"
        (per chunk of patches: one ``fine_clusters`` call of the scorer, ``fine_cluster.fine_clusters_f64`` on the
        GPU, then one read-back of the decisions and one copy of all heads; needs the HIP spot model).
        ``global_clustering``: where the global clustering decides -- "host" (the SI-SDR matrix, the segment tensor and
        the segment tables are read back and walked in numpy) or "device" (the three SI-SDR ops leave their results on
        the GPU, one ``global_clusters`` call of the scorer, ``global_cluster.global_clusters_f64`` on the GPU, decides
        there, and only the [n] labels come back; needs ``segments="device"`` and the HIP spot model).
        ``coarse``: where the coarse stage of a lattice search (``Prone_method`` in ``LATTICE_METHODS``) decides --
        "host" (a patch per cube, ``binary_search_baseline``) or "device" (``Apply_SRP_PHAT`` returns a lazy
        ``dense_grid.LatticePatches``; the offsets and distances of the cubes stay on the GPU as tables of the array,
        one ``score_offsets`` call, for "DENSE_NMS" one ``lattice_nms`` call on the device scores and one
        ``coarse_select`` call of the scorer, ``search.coarse_select_f64`` on the GPU, decide there, one read-back
        brings the decision, and only the kept patches are built; needs the HIP spot model on one GPU)."""
        # (an unknown Prone_method is refused below, whatever the modes are)
        modes = check_modes(geometry, segments, clustering, global_clustering, coarse,
                            Prone_method=Prone_method if Prone_method in PRONE_METHODS else None)
        for name, value in zip(MODE_NAMES[1:], modes[1:]):              # (``geometry`` goes to the SRP node below)
            setattr(self, name, value)
        if Prone_method not in PRONE_METHODS:
            # the reference silently keeps an all-zero map for an unknown name (sep/Mic_Array.py:165-170)
            raise ValueError(f"Prone_method must be one of {sorted(PRONE_METHODS)}, got {Prone_method!r}")
        self.Prone_method = Prone_method
        self.MIN_TRIGGER_POWER = MIN_TRIGGER_POWER
        self.visual_save = False
        self.Range_spk = Spk_Range
        print("Init the Range_spk: ", Spk_Range)
        self.mic_positions = mic_positions
        self.num_mic = mic_positions.shape[0]
        # physical TDoA bound per pair, 8 cm slack (sep/Mic_Array.py:114-116)
        self.upper_bound_pairwise = (np.linalg.norm(mic_positions[1:] - mic_positions[0], axis=1) + 0.08) \
            / SPEED_OF_SOUND * FS
        self.SRP_node = SRPPhat(mic_pos=mic_positions, freq_bins=FREQ_BINS, Range_spk=Spk_Range, grid_size=grid_size,
                                FS=FS, n_fft=N_FFT, threshold=[0.15, 0.015, 0.05], WIDTH=INIT_WIDTH, device=device,
                                geometry=geometry, lattice_width=INIT_WIDTH if Prone_method in LATTICE_METHODS else None)
        if Prone_method in LATTICE_METHODS and self.SRP_node.lattice.n_cubes == 0:
            raise RuntimeError("the keep-out region covers the whole speaker range: the TDoA lattice is empty")
        if coarse == "device":
            self.SRP_node.lattice_tables(mic_positions)     # once per array; the device copies follow at the first search
        self.original_times = 0
        self.spotforming_times = 0
        self.big_spotforming_times = 0
        self._device_scorer = None      # set by the fine stage when the spot model offers the GPU SI-SDR kernels
        self._seg_cache = {}
        self._dev_cache = {}
        # decision trace of the latest search (cheap bookkeeping, used by the precision flip-rate and
        # parity tests): coarse kept indices, per coarse patch {head: members} of the fine-stage
        # clustering, and the global clusters as lists of "g_head" names
        self.trace = {"coarse_kept": [], "fine_clusters": {}, "final_clusters": []}
        self.lattice_nms = None         # DENSE_NMS: radius, best and degree of the latest coarse stage

    # ---- stage 1: SRP-PHAT / MUSIC / TOPS pruning (sep/Mic_Array.py:152-194) --------------
    def Apply_SRP_PHAT(self, mix_data):
        self.SRP_node.reset()
        self.spotforming_times = 0
        self.original_times = 0
        if self.Prone_method in LATTICE_METHODS:
            # no map, so the mixture is not read and no window length is required; fresh Patch objects per call,
            # because check_out mutates them
            if self.coarse == "device":
                # nothing is built here: the cubes are rows of the array's tables until the coarse stage has decided
                offsets, dis1 = self.SRP_node.lattice_tables()
                return LatticePatches(self.SRP_node, self.SRP_node.lattice, offsets, dis1), np.zeros((3, 3))
            return lattice_patches(self.SRP_node, self.SRP_node.lattice), np.zeros((3, 3))
        mix_np = mix_data.numpy() if hasattr(mix_data, "numpy") else np.asarray(mix_data)
        win = 36000 if mix_np.shape[1] >= 72000 else 24000
        getattr(self.SRP_node, PRONE_METHODS[self.Prone_method])(mix_np, window=win)
        patch_list = self.SRP_node.local_source_adaptive()
        return patch_list, np.zeros((3, 3))

    # ---- stage 2: coarse Spotforming, relaxed window (sep/Mic_Array.py:196-222) ---------
    def Spotform_Big_Patch(self, mix_data, patch_list, spot_model):
        self.big_spotforming_times = len(patch_list)
        if self.coarse == "device":
            return self._coarse_device(mix_data, patch_list, spot_model)
        kept, _powers_with_dis, rel_thr = binary_search_baseline(
            mix_data, spot_model, patch_list, self.mic_positions,
            survivors=self._lattice_survivors if self.Prone_method == "DENSE_NMS" else None)
        self.Relative_Threshold = rel_thr
        pos = {id(p): i for i, p in enumerate(patch_list)}
        self.trace = {"coarse_kept": [pos[id(p)] for p in kept], "fine_clusters": {}, "final_clusters": []}
        return kept

    def _coarse_device(self, mix_data, patch_list, spot_model):
        """The coarse stage of a lattice search decided where the energies are: ``score_offsets`` on the array's offsets
        table, for "DENSE_NMS" ``lattice_nms`` on the device scores, ``coarse_select`` (``search.coarse_select_f64``),
        then the stage's one blocking copy -- kept, counts, threshold and, for the record in ``lattice_nms``, best and
        degree -- and a ``Patch`` for each kept cube only."""
        if getattr(spot_model, "world", 1) > 1:
            raise RuntimeError('coarse="device" runs on one GPU: a sharded spot model gathers its energies as host arrays')
        need_methods(spot_model, 'coarse="device"', "score_offsets", "coarse_select")
        if not isinstance(patch_list, LatticePatches):
            raise RuntimeError('coarse="device" takes the LatticePatches that Apply_SRP_PHAT returned')
        node = self.SRP_node
        dev = getattr(spot_model, "device", None)
        tables = node.lattice_tables_device("cpu" if dev is None else dev)
        offsets = patch_list.offsets_i32 if getattr(spot_model, "host_offsets", False) else tables["offsets"]
        en_dev = spot_model.score_offsets(mix_data, offsets, Strict=0)
        nms = self.Prone_method == "DENSE_NMS"
        radius = search.LATTICE_NMS_RADIUS
        best_dev = degree_dev = None
        if nms:
            best_dev, degree_dev = node.lattice_local_maxima_resident(en_dev[:, 1].contiguous(), radius)
        cap = search.MAX_BIG_PATCH
        kept_d, counts_d, thr_d = spot_model.coarse_select(en_dev, tables["dis1"], best_dev, cap=cap)
        kept_idx, counts, thr, *maxima = read_back(kept_d, counts_d, thr_d, *([best_dev, degree_dev] if nms else []))
        if nms:
            if counts[1] != 0:
                raise ValueError("every score must be finite")
            self.lattice_nms = {"radius": radius, "best": maxima[0], "degree": maxima[1]}
        if counts[0] > cap:
            print("warning too many patch remaining, only keep the best 30")
        self.Relative_Threshold = float(thr[0]) * 1.2
        kept_idx = [int(g) for g in kept_idx if g >= 0]
        self.trace = {"coarse_kept": kept_idx, "fine_clusters": {}, "final_clusters": []}
        return [patch_list[g] for g in kept_idx]

    def _lattice_survivors(self, powers_win):
        """DENSE_NMS: one flag per cube of the lattice, true for its local maxima under the windowed powers."""
        radius = search.LATTICE_NMS_RADIUS
        best, degree = self.SRP_node.lattice_local_maxima(powers_win, radius)
        self.lattice_nms = {"radius": radius, "best": best, "degree": degree}
        return best == np.arange(best.shape[0])

    # ---- stage 3: fine Spotforming, strict window (sep/Mic_Array.py:225-395) ------------
    def _subdivide(self, big):
        """Fine candidates of one coarse patch: its hypercube subdivision plus the centre
        candidate, which goes last (sep/Mic_Array.py:245-262)."""
        P = self.num_mic - 1
        fine = search_area([big], self.mic_positions, self.upper_bound_pairwise)
        centre_patch = Patch(big.sample_offset, [2 for _ in range(P)], None, big.peak_pos)
        c = centre_patch.center_pos()
        if c is not None:
            fine.append(centre_patch)
        else:
            print("it is impossible to be here")
        return fine, c

    def _cluster_group(self, g, big, patches, powers, powers2, area, centre, T_len, thr_new, sample_gt,
                       sim_of, audio_of):
        """Thresholding + SI-SDR clustering of the candidates of ONE coarse patch and the output
        tuples of its cluster heads (sep/Mic_Array.py:283-383).  ``sim_of(k, h)`` gives
        si_sdr(candidate k, candidate h); ``audio_of(heads)`` the heads' waveforms."""
        big_label = self._big_label(big, sample_gt)
        if np.amax(powers2) < self._group_gate(big, thr_new):
            return []
        order = np.argsort(-1 * np.array(powers))                           # sorted by total power (:339)
        clusters = {}
        # the reference scales the trigger by the length of the LAST candidate row (:343)
        min_trigger = self.MIN_TRIGGER_POWER / (3 * 48000) * T_len
        for k in order:
            d = np.linalg.norm(patches[k].center_pos() - self.mic_positions[0])
            if powers2[k] < thr_new / (1 + d) or powers[k] < min_trigger:
                continue
            home = None
            for head in clusters:
                if sim_of(k, clusters[head][0]) > -4:                       # SI_SDR_THRESHOLD (:340)
                    home = head
                    break
            if home is None:
                clusters[k] = [k]
            else:
                clusters[home].append(k)
        return self._cluster_outputs(g, patches, powers, clusters, area, centre, big_label, audio_of)

    @staticmethod
    def _big_label(big, sample_gt):
        """Index of the ground-truth source within 3.5 samples of the coarse patch, or -1 (sep/Mic_Array.py:283-289)."""
        if sample_gt is not None:
            for k in range(sample_gt.shape[1]):
                if np.amax(np.abs(big.sample_offset - sample_gt[:, k])) < 3.5:
                    return k
        return -1

    def _group_gate(self, big, thr_new):
        """The level the best candidate of a coarse patch must reach for the patch to be clustered at all."""
        c = big.center_pos()
        d = np.linalg.norm(c - self.mic_positions[0]) if c.shape[0] == 3 else 4
        return thr_new / (1 + d)

    def _cluster_outputs(self, g, patches, powers, clusters, area, centre, big_label, audio_of):
        """The tail of ``_cluster_group`` both clustering modes share: the trace entry of an open coarse patch and the
        output tuples of its cluster heads.  ``clusters`` = {head: members}, heads in creation order, members in
        visiting order (``weight_mean_pos`` sums in that order)."""
        out = []
        self.trace["fine_clusters"][int(g)] = {int(h): [int(k) for k in m] for h, m in clusters.items()}
        if len(clusters) == 0:
            return out
        heads = list(clusters.keys())
        audio = audio_of(heads)
        area_samples = None
        for n, head in enumerate(heads):
            _position, offs = weight_mean_pos(patches, powers, clusters[head])
            if area_samples is None:                                        # once per coarse patch
                area_samples = pair_offsets(area, self.mic_positions, SPEED_OF_SOUND, FS)
            merged = find_merge_center(offs, area, self.mic_positions, centre, area_samples)
            if merged.center_pos() is None:
                print("Warning some bug happen one source may be drop")
            out.append((merged, audio[n], powers[head], str(g) + '_' + str(head),
                        {"audio_offset": patches[head].sample_offset, "localization_offset": offs}, big_label))
        return out

    def _resident_group(self, g, big, patches, waves_g, energies_g, area, centre, T_len, thr_new, sample_gt,
                        spot_model):
        """One coarse patch with the waveforms on the GPU: similarities from one Gram launch (made
        only if a second candidate survives the thresholds), heads copied to the host."""
        sim = {}

        def sim_of(k, h):
            if "m" not in sim:
                sim["m"] = spot_model.pair_sisdr(waves_g)
            return sim["m"][k, h]

        kept = {}

        def audio_of(heads):
            kept["rows"] = waves_g[heads]
            return kept["rows"].cpu().numpy()
        out = self._cluster_group(g, big, patches, list(energies_g[:, 0]), list(energies_g[:, 1]), area, centre,
                                  T_len, thr_new, sample_gt, sim_of, audio_of)
        self._register_heads(out, kept.get("rows", ()))
        return out

    def _register_heads(self, pairs, rows_dev):
        """What the global clustering needs of the heads the fine stage just copied to the host: their voiced
        segments, found here while they hide behind the GPU (``segments="device"``: not here, the clustering finds all
        heads' segments in one launch), and ``rows_dev``, the same waveforms still on the GPU."""
        assert len(pairs) == len(rows_dev)
        for pair, row in zip(pairs, rows_dev):
            if self.segments != "device":
                self._seg_cache[id(pair[1])] = (pair[1], split_wav(pair[1]))
            self._dev_cache[id(pair[1])] = (pair[1], row)

    def _fine_gates(self, bigs, fines, thr_new):
        """(bounds [G+1], gate [N], group_gate [G]) of a chunk of coarse patches for ``fine_clusters``: the very
        thresholds ``_cluster_group`` forms, which depend on the patch geometry and ``thr_new`` only."""
        bounds = np.zeros(len(fines) + 1, dtype=np.int32)
        bounds[1:] = np.cumsum([len(f) for f in fines])
        gate = np.empty(int(bounds[-1]), dtype=np.float64)
        k = 0
        for fine in fines:
            for p in fine:
                d = np.linalg.norm(p.center_pos() - self.mic_positions[0])
                gate[k] = thr_new / (1 + d)
                k += 1
        group_gate = np.array([self._group_gate(big, thr_new) for big in bigs], dtype=np.float64).reshape(-1)
        return bounds, gate, group_gate

    def _device_groups(self, groups, bigs, fines, centres, waves, en_dev, gates, T_len, sample_gt, scorer):
        """A chunk of coarse patches with the waveforms on the GPU and the clustering there too: one
        ``fine_clusters`` call, one read-back of (energies, order, label), one gather and copy of all heads' rows;
        then the bookkeeping of ``_cluster_group`` per patch.  -> (output tuples, host energies [N, 2])."""
        import torch
        bounds, gate, group_gate = gates
        # the reference scales the trigger by the length of the LAST candidate row (:343)
        min_trigger = self.MIN_TRIGGER_POWER / (3 * 48000) * T_len
        order_d, label_d = scorer.fine_clusters(waves, bounds, en_dev, gate, group_gate, min_trigger)
        energies, order, label = read_back(en_dev, order_d, label_d)
        opened = []                                        # (position in the chunk, clusters) of the open patches
        head_rows = []
        for i in range(len(groups)):
            b0, n = int(bounds[i]), int(bounds[i + 1] - bounds[i])
            if n == 0 or np.amax(energies[b0:b0 + n, 1]) < group_gate[i]:
                continue
            clusters = clusters_of_group(order, label, b0, n)
            opened.append((i, clusters))
            head_rows.extend(b0 + h for h in clusters)
        rows_dev = rows = ()                               # (a chunk whose open patches have no head copies nothing)
        if head_rows:
            idx = torch.from_numpy(np.asarray(head_rows, dtype=np.int64))
            if waves.is_cuda:
                idx = idx.pin_memory().to(waves.device, non_blocking=True)
            rows_dev = waves.index_select(0, idx)
            rows = rows_dev.cpu().numpy()
        out, pos = [], 0
        for i, clusters in opened:
            b0, n = int(bounds[i]), int(bounds[i + 1] - bounds[i])
            first = pos
            pos += len(clusters)
            pairs = self._cluster_outputs(groups[i], fines[i], list(energies[b0:b0 + n, 0]), clusters,
                                          bigs[i].area_points, centres[i], self._big_label(bigs[i], sample_gt),
                                          lambda heads, first=first: rows[first:first + len(heads)])
            self._register_heads(pairs, rows_dev[first:pos])
            out.extend(pairs)
        return out, energies

    def _cluster_chunk(self, groups, bigs, fines, centres, waves, en_dev, gates, T_len, thr_new, sample_gt, spot_model):
        """The clustering of one chunk of coarse patches ``groups`` (``bigs``, their subdivisions ``fines`` and
        ``centres``) whose candidates' waveforms ``waves`` [N, T] and energies ``en_dev`` [N, 2] are on the GPU.
        ``gates`` (``_fine_gates``) says the clustering is on the device: one ``_device_groups`` call; with None the
        energies are read back and the patches go through ``_resident_group`` one by one.
        -> (output tuples, host energies [N, 2])."""
        if gates is not None:
            return self._device_groups(groups, bigs, fines, centres, waves, en_dev, gates, T_len, sample_gt,
                                       getattr(spot_model, "inner", spot_model))
        energies = en_dev.cpu().numpy()
        out, pos = [], 0
        for g, big, fine, centre in zip(groups, bigs, fines, centres):
            n = len(fine)
            out.extend(self._resident_group(g, big, fine, waves[pos:pos + n], energies[pos:pos + n], big.area_points,
                                            centre, T_len, thr_new, sample_gt, spot_model))
            pos += n
        return out, energies

    def _gather_pairs(self, output_pair, spot_model):
        """The sharded fine stage's last exchange: every rank's output tuples, in one order on all of them.  The voiced
        segments of every head travel with its tuple: the global clustering of every rank then finds them cached for
        the remote heads too, as it does for its own (segments="device": the cache is empty, None travels in their
        place and every rank finds them on its GPU)."""
        tagged = [p + (self._seg_cache.get(id(p[1]), (None, None))[1],) for p in output_pair]
        merged = spot_model.gather_pairs(tagged)
        output_pair = [t[:-1] for t in merged]
        for t, p in zip(merged, output_pair):
            if t[-1] is not None:
                self._seg_cache[id(p[1])] = (p[1], t[-1])
        return output_pair

    def Spotform_Small_Patch_Parallel(self, mix_data, candidate_finished, spot_model, sample_gt=None,
                                      run_demo_folder=None):
        thr_new = min([SPOT_POWER_THRESHOLD2, self.Relative_Threshold]) if USE_RELATIVE_SPOT_POWER \
            else SPOT_POWER_THRESHOLD2
        resident = hasattr(spot_model, "shift_and_sep_resident")
        inner = getattr(spot_model, "inner", spot_model)                 # ShardedSpotModel wraps the scorer
        self._device_scorer = inner if (resident and hasattr(inner, "segment_sisdr")) else None
        if self.segments == "device":
            need_methods(self._device_scorer, 'segments="device"', "voiced_segments")
        on_device = self.clustering == "device"
        if on_device:                                      # (the reference's host loops below cannot serve it either)
            need_methods(inner if resident else None, 'clustering="device"', "fine_clusters")
        sharded = getattr(spot_model, "world", 1) > 1
        n_groups = len(candidate_finished)
        self.spotforming_times = 0
        self._seg_cache = {}               # id(waveform) -> (waveform, voiced segments), filled by the resident path
        self._dev_cache = {}               # id(waveform) -> (waveform, its device row)
        if resident and not sharded and n_groups >= 3 and getattr(spot_model, "device", None) is not None:
            return self._fine_stage_pipelined(mix_data, candidate_finished, spot_model, sample_gt, thr_new)
        if resident and sharded and getattr(inner, "device", None) is not None:
            return self._fine_stage_sharded(mix_data, candidate_finished, spot_model, sample_gt, thr_new)

        subdivided, centers, bounds = [], [], [0]
        for big in candidate_finished:
            fine, c = self._subdivide(big)
            subdivided.append(fine)
            centers.append(c)
            self.spotforming_times += len(fine)
            bounds.append(self.spotforming_times)

        # one rank per GPU (shard.ShardedSpotModel): whole coarse patches are dealt to ranks so
        # the per-patch clustering below stays local; energies are all-gathered (the stage's one
        # collective) and only the finished output tuples travel.
        mine = spot_model.my_groups([len(fine) for fine in subdivided]) if sharded else list(range(n_groups))
        bigs, fines, centres = ([seq[g] for g in mine] for seq in (candidate_finished, subdivided, centers))
        flat = [p for fine in fines for p in fine]             # this rank's candidates

        # the hot call.  With the HIP spot model the N x T outputs stay on the GPU: energies come
        # from the device reduction, SI-SDR similarities from the device Gram kernel, and only
        # the cluster heads' waveforms are copied to the host: this rank's patches
        # are one chunk of ``_cluster_chunk``.  Any other duck-typed model goes through the
        # reference's host loops.
        output_pair = []
        if resident:
            if flat:
                waves, en_dev = spot_model.shift_and_sep_resident(mix_data, flat, Strict=1, device_energies=True)
                gates = self._fine_gates(bigs, fines, thr_new) if on_device else None
                output_pair, energies = self._cluster_chunk(list(mine), bigs, fines, centres, waves, en_dev, gates,
                                                            int(waves.shape[1]), thr_new, sample_gt, spot_model)
            else:                                              # a rank that was dealt no coarse patch asks nothing
                output_pair, energies = [], np.zeros((0, 2))
            if sharded:
                self.fine_energies = spot_model.all_gather_groups(energies, mine, bounds)
        elif flat:
            sep_all = spot_model.shift_and_sep(mix_data, flat, Strict=1)
            T_len = int(sep_all.shape[1])
            pos = 0
            for g, big, patches, centre in zip(mine, bigs, fines, centres):
                sep = sep_all[pos:pos + len(patches)]
                pos += len(patches)
                powers, powers2 = mean_removed_energies(sep, in_place=True)    # in place, as :291: the heads' audio
                output_pair.extend(self._cluster_group(
                    g, big, patches, powers, powers2, big.area_points, centre, T_len, thr_new, sample_gt,
                    lambda k, h, sep=sep: si_sdr(sep[k, :], sep[h]), lambda heads, sep=sep: [sep[h, :] for h in heads]))
        return self._gather_pairs(output_pair, spot_model) if sharded else output_pair

    def _fine_stage_sharded(self, mix_data, candidate_finished, spot_model, sample_gt, thr_new):
        """One rank per GPU with the HIP model (shard.ShardedSpotModel).  Whole coarse patches are dealt to
        ranks by a weight every rank knows without subdividing anything -- the number of 1 cm grid points of
        the patch, which is what drives the size of its subdivision; each rank then subdivides and runs the
        pipelined fine stage on ITS patches only.  The stage's exchanges follow: the sizes (a few integers),
        the energy all-gather, and the object gather of the finished output tuples with their voiced
        segments.  Same output_pair list on every rank as on one GPU."""
        n_groups = len(candidate_finished)
        owners = spot_model.deal_groups([max(1, big.area_size()) for big in candidate_finished])
        mine = owners[spot_model.rank]
        sizes_mine = {}
        output_pair, energies = self._fine_stage_pipelined(mix_data, candidate_finished, spot_model, sample_gt, thr_new,
                                                           owned=mine, sizes_out=sizes_mine)
        sizes = spot_model.gather_sizes(sizes_mine, n_groups)
        self.spotforming_times = int(sum(sizes))
        gbounds = [0]
        for n in sizes:
            gbounds.append(gbounds[-1] + n)
        self.fine_energies = spot_model.all_gather_groups(energies, mine, gbounds, owners=owners)
        return self._gather_pairs(output_pair, spot_model)

    def _fine_stage_pipelined(self, mix_data, candidate_finished, spot_model, sample_gt, thr_new, owned=None, sizes_out=None):
        """Single-GPU fine stage with the host work hidden behind the GPU: the coarse patches are
        processed in contiguous chunks; while the GPU evaluates the candidates of chunk c
        the host subdivides the patches of chunk c+1, and the clustering of chunk c (energies,
        Gram launches, head copies -- issued on a side stream that only waits for chunk c) runs
        while the GPU is already on chunk c+1.  Same candidates, same order, same output.
        With ``clustering="device"`` the clustering of chunk c is one ``fine_clusters`` call and two read-backs.
        ``owned`` (sharded use): the coarse patches this rank owns; the call then returns (output_pair,
        energies of these groups in that order) and reports their subdivision sizes in ``sizes_out``."""
        import torch
        dev = getattr(spot_model, "inner", spot_model).device
        on_device = self.clustering == "device"
        mix_dev = torch.as_tensor(mix_data).to(dev, dtype=torch.float32).contiguous()
        T_len = int(mix_dev.shape[1])
        order = list(range(len(candidate_finished))) if owned is None else [int(g) for g in owned]
        n_groups = len(order)
        local_energies = []
        if n_groups == 0:                                  # a rank that was dealt no coarse patch
            return ([], np.zeros((0, 2))) if owned is not None else []
        if getattr(self, "_side_stream", None) is None:
            # high priority: its SI-SDR kernels and read-backs are tiny and sit on the search's critical path, while the
            # main stream is running whole network launches that fill the device
            self._side_stream = torch.cuda.Stream(device=dev, priority=-1)
        side, main = self._side_stream, torch.cuda.current_stream(dev)
        # Chunk edges (fractions of the coarse patches).  Only two pieces of host work cannot hide behind
        # the GPU: the subdivision of the first chunk and the clustering of the last one -- so those two
        # chunks are small (about 1/15 of the patches each) and the middle ones large enough to keep the
        # internal batches full.  (Bench scene, 710 candidates, same box: three equal chunks 361 ms; these
        # edges 340; [0, .1, .5, .9, 1] 346; [0, .13, .5, .87, 1] 349; seven chunks 345.)
        edges = sorted(set(min(n_groups, max(0, round(n_groups * f))) for f in FINE_CHUNK_EDGES) | {0, n_groups})
        n_chunks = len(edges) - 1
        output_pair, inflight = [], None

        def finish(job):
            groups, fines, centres, waves, en_dev, ev, gates = job
            with torch.cuda.stream(side):
                side.wait_event(ev)
                waves.record_stream(side)
                en_dev.record_stream(side)
                pairs, energies = self._cluster_chunk(groups, [candidate_finished[g] for g in groups], fines, centres,
                                                      waves, en_dev, gates, T_len, thr_new, sample_gt, spot_model)
            output_pair.extend(pairs)
            local_energies.append(energies)

        for k in range(n_chunks):
            groups = order[edges[k]:edges[k + 1]]
            if not groups:
                continue
            fines, centres, flat = [], [], []
            for g in groups:                                   # host: subdivision of this chunk
                fine, c = self._subdivide(candidate_finished[g])
                self.spotforming_times += len(fine)
                if sizes_out is not None:
                    sizes_out[int(g)] = len(fine)
                fines.append(fine)
                centres.append(c)
                flat.extend(fine)
            waves, en_dev = spot_model.shift_and_sep_resident(mix_dev, flat, Strict=1, device_energies=True)
            ev = torch.cuda.Event()
            ev.record(main)
            # (device clustering: the thresholds are geometry alone, formed while the GPU runs this chunk)
            gates = self._fine_gates([candidate_finished[g] for g in groups], fines, thr_new) if on_device else None
            if inflight is not None:
                finish(inflight)                               # host clustering of the previous chunk
            inflight = (groups, fines, centres, waves, en_dev, ev, gates)
        if inflight is not None:
            finish(inflight)
        if owned is not None:
            return output_pair, (np.concatenate(local_energies, axis=0) if local_energies else np.zeros((0, 2)))
        return output_pair

    # ---- stage 4: global non-max suppression (sep/Mic_Array.py:399-500) -----------------
    @staticmethod
    def _near_matrix(centres):
        """dis < 0.45 for every ordered pair of the (x, y) centres; entries within rounding of the threshold are settled
        by the very call the per-pair form makes."""
        xy = np.array([c[:2] for c in centres], dtype=np.float64)
        d = xy[:, None, :] - xy[None, :, :]
        dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        near = dist < 0.45
        for a, b in zip(*np.nonzero(np.abs(dist - 0.45) < 1e-9)):
            near[a, b] = np.linalg.norm(centres[a][:2] - centres[b][:2]) < 0.45
        return near

    def _candidate_rows(self, cands, scorer):
        """The candidates' waveforms as one device tensor [n, T]: the rows the fine stage left on the GPU, or a copy."""
        import torch
        dev_rows = [getattr(self, "_dev_cache", {}).get(id(c[1])) for c in cands]
        if all(r is not None and r[0] is c[1] for r, c in zip(dev_rows, cands)):
            return torch.stack([r[1] for r in dev_rows])          # the fine stage left every row on the GPU
        waves = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(c[1], dtype=np.float32) for c in cands])))
        return waves.to(scorer.device if getattr(scorer, "device", None) is not None else "cuda")

    def _global_clusters_device(self, cands, centres, scorer, sample_gt):
        """``Clustering_new`` with the decisions made where the SI-SDR tensors are: four calls are enqueued, nothing of
        theirs is read back, and the stage's one blocking copy is the [n] labels of ``global_clusters``
        (``global_cluster.global_clusters_f64``: -1 discarded, -2 shadowed, otherwise the head's row)."""
        n = len(cands)
        waves = self._candidate_rows(cands, scorer)
        near = self._near_matrix(centres).astype(np.uint8)
        seg_tab_dev, cnt_dev = scorer.voiced_segments(waves)
        full_dev = scorer.pair_sisdr_device(waves)
        seg_dev = scorer.segment_sisdr_resident(waves, seg_tab_dev, cnt_dev)
        label = scorer.global_clusters(full_dev, seg_dev, cnt_dev, near).cpu().numpy()
        wrong = []
        for i in range(n):
            h = int(label[i])
            if h == -1:
                print("discard because no invalid split!!!")
            elif h >= 0 and h != i and cands[i][-1] >= 0 and sample_gt is not None and cands[h][-1] == -1:
                delta = (cands[h][-2]["audio_offset"] - sample_gt[:, cands[i][-1]]).astype(int)
                wrong.append((cands[i][-1], cands[h][-1], delta, cands[i][2] / cands[h][2]))
        return self._final_clusters(cands, clusters_of_labels(label), wrong)

    def _final_clusters(self, cands, clusters, wrong):
        """What ``Clustering_new`` returns for ``clusters`` = {head: members, the head first} over the sorted candidates,
        heads in creation order; records them in the trace."""
        print("final speaker number is ", len(clusters.keys()))
        self.trace["final_clusters"] = [[cands[i][3] for i in clusters[h]] for h in clusters]
        patch_final = [cands[clusters[h][0]] for h in clusters]
        audio_final = [p[1] for p in patch_final]
        return audio_final, patch_final, self.big_spotforming_times + self.spotforming_times, wrong

    def Clustering_new(self, output_pair, simple_pos=None, sample_gt=None):
        cands = sorted(output_pair, key=lambda x: -x[2])
        # With the HIP spot model the O(n^2) waveform comparisons of this stage run on the GPU:
        # one launch for the full-length SI-SDR matrix, one for the segment-wise tensor
        # (SURVEY.md §8f-2).  Any other model keeps the reference's host loops.
        scorer = getattr(self, "_device_scorer", None)
        cache = getattr(self, "_seg_cache", {})
        on_device = self.segments == "device"
        if on_device:
            need_methods(scorer, 'segments="device"', "voiced_segments")
        if self.global_clustering == "device":
            need_methods(scorer, 'global_clustering="device"', "global_clusters")
            centres = [c[0].center_pos() for c in cands]
            if len(cands) > 0 and all(c is not None for c in centres):
                return self._global_clusters_device(cands, centres, scorer, sample_gt)
            # (a candidate without a centre: the per-pair loop below, as in host mode)
        seg_all = []
        for c in ([] if on_device else cands):
            hit = cache.get(id(c[1]))
            seg_all.append(hit[1] if hit is not None and hit[0] is c[1] else split_wav(c[1]))
        full_dev = seg_dev = None
        if scorer is not None and (len(cands) > 1 or (on_device and len(cands) > 0)):
            waves = self._candidate_rows(cands, scorer)
            if on_device:
                # one launch pair finds every head's segments; the tables stay where segment_sisdr reads them and
                # only they (a few KB) come back, for len(segs) and the seg_tab slices below
                seg_tab_dev, cnt_dev = scorer.voiced_segments(waves)
                if len(cands) > 1:
                    full_dev = scorer.pair_sisdr(waves)
                    seg_dev, cnt = scorer.segment_sisdr_device(waves, seg_tab_dev, cnt_dev)
                else:
                    cnt = cnt_dev.cpu().numpy()
                seg_host = seg_tab_dev.cpu().numpy()
                seg_all = [seg_host[i, :int(cnt[i])] for i in range(len(cands))]
            else:
                full_dev = scorer.pair_sisdr(waves)
                seg_dev, _ = scorer.segment_sisdr(waves, seg_all)
        clusters = {}
        wrong = []
        centres = [c[0].center_pos() for c in cands]
        win_dev = None
        if seg_dev is not None:
            # check_sisnr_win of every ordered pair at once (entries beyond a candidate's own segment
            # count are NaN and compare false, like the slice [:len(segs)] of the per-pair form)
            with np.errstate(invalid="ignore"):
                win_dev = np.any(seg_dev > -2, axis=2) & ~np.any(seg_dev < -7, axis=2)
        near = None
        if win_dev is not None and all(c is not None for c in centres):
            near = self._near_matrix(centres)                    # dis < 0.45 for every pair
            merge = (full_dev > -1) | win_dev | near             # (:401,458) for every ordered pair
        heads = []                                               # cluster heads in creation order
        for i, cand in enumerate(cands):
            centre1, audio1, power1, big_label = centres[i], cand[1], cand[2], cand[-1]
            segs = seg_all[i]
            if len(segs) == 0:
                print("discard because no invalid split!!!")
                continue
            unique, belong = True, -1
            seg_tab, seen = [], []
            if near is not None:
                hit = np.flatnonzero(merge[i, heads]) if heads else np.empty(0, dtype=np.int64)
                if hit.size:                                     # first head in creation order wins
                    belong = heads[int(hit[0])]
                    clusters[belong].append(i)
                    unique = False
                    seen = heads[:int(hit[0]) + 1]
                else:
                    seen = list(heads)
            else:
                for head in clusters:
                    h = clusters[head][0]
                    audio2, centre2 = cands[h][1], centres[h]
                    sim = si_sdr(audio1, audio2)
                    per_seg = split_wise_sisdr(audio1, audio2, segs)
                    seg_tab.append(per_seg)
                    dis = np.linalg.norm(centre1[:2] - centre2[:2])
                    if sim > -1 or check_sisnr_win(per_seg) or dis < 0.45:      # (:401,458)
                        clusters[h].append(i)
                        unique, belong = False, head
                        break
            if seen:
                seg_tab = seg_dev[i, seen, :len(segs)]
            if len(seg_tab) != 0:
                best = np.amax(np.array(seg_tab), axis=0)
                if check_sisnr_win(best, SISNR_THRESHOLD=-1, SISNR_THRESHOLD2=-5):
                    unique = False
            if unique:
                clusters[i] = [i]
                heads.append(i)
            elif big_label >= 0 and sample_gt is not None and belong >= 0:
                h = clusters[belong][0]
                if cands[h][-1] == -1:
                    delta = (cands[h][-2]["audio_offset"] - sample_gt[:, big_label]).astype(int)
                    wrong.append((big_label, cands[h][-1], delta, power1 / cands[h][2]))
        return self._final_clusters(cands, clusters, wrong)
