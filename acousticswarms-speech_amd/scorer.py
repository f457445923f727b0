"""The device helpers of the search that need no network: SI-SDR matrices, voiced segments and the three decision
kernels, each one ``torch.ops.asw.*`` call on the caller's tensors (csrc/torch_ops.cpp).  ``DeviceScorer(device)`` stands
on its own; ``spot.SpotModel`` inherits it, so a spot model is still the scorer ``MicArray`` asks for by ``hasattr``
(``modes.need_methods``), and ``batching.MixtureScorer`` forwards exactly ``DeviceScorer.HELPERS``.  A further device
stage is a method here and its name in that tuple.
"""
import numpy as np

from . import native


class DeviceScorer:
    # the public names, said once (``MixtureScorer.FORWARDED`` is this tuple)
    HELPERS = ("pair_sisdr", "segment_sisdr", "voiced_segments", "segment_sisdr_device", "fine_clusters",
               "pair_sisdr_device", "segment_sisdr_resident", "global_clusters", "coarse_select")

    def __init__(self, device=None):
        """``device``: where the caller's tensors live (kept as ``self.device`` for ``MicArray``; every method runs on
        the device of the tensors it is given)."""
        if device is not None:
            import torch
            device = torch.device(device)
        self.device = device

    # ---- the two SI-SDR ops ----------------------------------------------------------------
    @staticmethod
    def _pair(waves):
        return native.torch_ops().pair_sisdr(waves.contiguous())

    @staticmethod
    def _segment(waves, seg_dev, cnt_dev):
        return native.torch_ops().segment_sisdr(waves.contiguous(), seg_dev.contiguous(), cnt_dev.contiguous())

    def pair_sisdr(self, waves):
        """SI-SDR matrix S[i][j] = si_sdr(est=waves[i], ref=waves[j]) computed on the GPU
        (sep/helpers/eval_utils.py:11-39); returns a host ndarray [n,n] float64."""
        return self._pair(waves).cpu().numpy()

    def pair_sisdr_device(self, waves):
        """``pair_sisdr`` whose result stays where it was written: the device tensor [n,n] float64.  Nothing is copied
        and nothing waits for the device."""
        return self._pair(waves)

    def segment_sisdr(self, waves, segments):
        """Segment-wise SI-SDR tensor S[i][j][k] = si_sdr(waves[i][seg_k(i)], waves[j][seg_k(i)])
        on the GPU (split_wise_sisdr, sep/helpers/eval_utils.py:73-82): ``segments[i]`` is the
        list of [start, end) of waveform i (split_wav).  Returns (host ndarray [n,n,kmax]
        float64, counts [n]); entries beyond a waveform's segment count are NaN."""
        import torch
        n, T = waves.shape
        cnt = np.array([len(s) for s in segments], dtype=np.int32)
        kmax = max(1, int(cnt.max()) if n else 1)
        seg = np.zeros((n, kmax, 2), dtype=np.int32)
        for i, sl in enumerate(segments):
            for k, (a, b) in enumerate(sl):
                if not (0 <= a <= b <= T):
                    raise RuntimeError(f"segment [{a},{b}) of waveform {i} lies outside [0,{T}]")
                seg[i, k] = (a, b)
        out = self._segment(waves, torch.from_numpy(seg).to(waves.device), torch.from_numpy(cnt).to(waves.device))
        return out.cpu().numpy(), cnt

    def segment_sisdr_device(self, waves, seg_dev, cnt_dev):
        """``segment_sisdr`` on tables that are already on the device (``voiced_segments``): the same op, the same
        return -- (host ndarray [n,n,kmax] float64 with kmax = max(1, largest count), counts [n]).  Only the counts
        come to the host before the launch: they size the result, so the slots no waveform uses are not computed,
        filled with NaN and read back."""
        cnt = cnt_dev.cpu().numpy()
        kmax = max(1, int(cnt.max()) if cnt.size else 1)
        return self._segment(waves, seg_dev[:, :kmax], cnt_dev).cpu().numpy(), cnt

    def segment_sisdr_resident(self, waves, seg_tab_dev, cnt_dev):
        """``segment_sisdr`` on the device tables of ``voiced_segments`` whose result stays on the device: the tensor
        [n,n,kcap] float64, kcap the table's own width (NaN beyond a waveform's count), so that no count has to come
        to the host to size it.  Nothing is copied and nothing waits for the device."""
        return self._segment(waves, seg_tab_dev, cnt_dev)

    # ---- segments and decisions ---------------------------------------------------------------
    def voiced_segments(self, waves, top_db: float = 18.0):
        """The voiced segments of every row of ``waves`` (device tensor [n,T] float32) found on the GPU
        (``hostdsp.voiced_segments_f64``, the float64 statement of ``split_wav``): returns the device tensors
        (segments [n, max(1, T//1000), 2] int32 with [0, 0] beyond a row's count, counts [n] int32).  Nothing is
        copied and nothing waits for the device."""
        seg, cnt, _ms = native.torch_ops().voiced_segments(waves.contiguous(), float(top_db), False)
        return seg, cnt

    def fine_clusters(self, waves, bounds, en_dev, gate, group_gate, min_trigger, sim_db: float = -4.0):
        """The fine stage's clustering of every group of rows of ``waves`` (device tensor [N,T] float32) on the GPU
        (``fine_cluster.fine_clusters_f64``): ``bounds`` host ints [G+1], ``en_dev`` the device energies [N,2] float64,
        ``gate`` [N] and ``group_gate`` [G] host float64.  Returns the device tensors (order [N] int32, label [N]
        int32).  The bounds and the gates (a few KB) go up through pinned memory; nothing comes back and nothing
        waits for the device."""
        import torch
        b = torch.from_numpy(np.ascontiguousarray(bounds, dtype=np.int32))
        gates = np.concatenate([np.asarray(gate, dtype=np.float64).reshape(-1),
                                np.asarray(group_gate, dtype=np.float64).reshape(-1)])
        gates_d = torch.from_numpy(gates).pin_memory().to(waves.device, non_blocking=True)
        n = int(waves.shape[0])
        order, label, _gram = native.torch_ops().fine_clusters(waves.contiguous(), b, en_dev.contiguous(), gates_d[:n],
                                                               gates_d[n:], float(min_trigger), float(sim_db), False)
        return order, label

    def global_clusters(self, full_dev, seg_dev, cnt_dev, near_host_u8):
        """The global clustering's decisions on the GPU (``global_cluster.global_clusters_f64``) over the device
        tensors of ``pair_sisdr_device``, ``segment_sisdr_resident`` and ``voiced_segments``; ``near_host_u8`` is the
        host's uint8 [n,n] ``dis < 0.45`` matrix and goes up through pinned memory.  Returns the device tensor label
        [n] int32; nothing comes back and nothing waits for the device."""
        import torch
        near = torch.from_numpy(np.ascontiguousarray(near_host_u8, dtype=np.uint8))
        near_d = near.pin_memory().to(full_dev.device, non_blocking=True)
        label, _merge = native.torch_ops().global_clusters(full_dev.contiguous(), seg_dev.contiguous(),
                                                           cnt_dev.contiguous(), near_d)
        return label

    def coarse_select(self, en_dev, dis1_dev, best_dev=None, thr1=None, relative=None, rel: float = 0.4, cap=None):
        """The coarse stage's decision on the GPU (``search.coarse_select_f64``) over the device energies [N,2] of
        ``score_offsets``, the device table ``dis1_dev`` [N] and, for the lattice's local maxima, ``best_dev`` int32 [N]
        of ``lattice_nms``.  The thresholds default to ``search``'s constants, read per call.  Returns the device
        tensors (kept [cap] int32 with -1 in the unused slots, counts [2] int32 = (cubes that pass, powers that are not
        finite), thr [2] float64 = (threshold, largest weighted power)); nothing comes back and nothing waits for the
        device."""
        from . import search
        return native.torch_ops().coarse_select(
            en_dev.contiguous(), dis1_dev.contiguous(), None if best_dev is None else best_dev.contiguous(),
            float(search.SPOT_POWER_THRESHOLD1 if thr1 is None else thr1),
            bool(search.USE_RELATIVE_SPOT_POWER if relative is None else relative), float(rel),
            int(search.MAX_BIG_PATCH if cap is None else cap))
