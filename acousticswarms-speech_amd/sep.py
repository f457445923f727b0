"""Host-side mirror of the joint separation network's call surface over libasw_hip.so.

``SepModel`` keeps the names, argument meaning and return types of the reference ``Network``
(sep/training/SpeakerSeparation/network.py:323-548): ``infer(input_channels, patch_list)``,
``infer_sample(input_channels, sample_list)`` -> ndarray [S, T], and ``forward(mix,
num_speakers)`` on already normalised input.  It is what ``JointModel.sep_model`` holds
(sep/training/JointModel/network.py:122,201-209).  ``infer_batch(mixes, sample_lists)`` is ``infer_sample`` over a batch
of mixtures in packed device calls (no counterpart in the reference).  All arithmetic runs in the HIP library,
reached through ``torch.ops.asw.sep_infer`` / ``sep_forward``; PyTorch is used for device
memory and streams only.  There is no CPU path.
"""
import numpy as np

from . import native
from .config import SEP_FULL, SepConfig, sep_param_shapes
from .device_model import DeviceModel

MAX_SEQUENCES = 64       # S (or B*S) per library call


def rounded_offsets(sample_list, n_pairs: int) -> np.ndarray:
    """np.round on the float64 offsets, as :507 does (half to even), -> int32 [S, M-1]."""
    if len(sample_list) == 0:
        return np.zeros((0, n_pairs), dtype=np.int32)
    offs = np.stack([np.asarray(s, dtype=np.float64) for s in sample_list])
    if offs.ndim != 2 or offs.shape[1] != n_pairs:
        raise RuntimeError(f"speaker has {offs.shape[-1]} offsets, mixture has {n_pairs + 1} channels")
    return np.round(offs).astype(np.int32)


def pack_items(counts, cap: int = MAX_SEQUENCES):
    """The device calls of a batch: items stay whole and in order, and every call takes as many as fit ``cap``
    sequences.  -> list of (first, last) item ranges, ``last`` exclusive, covering every item once (an item with no
    sequence rides along with its neighbours).  An item wider than ``cap`` raises ``RuntimeError``."""
    calls, first, total = [], 0, 0
    for k, c in enumerate(counts):
        c = int(c)
        if c < 0:
            raise ValueError(f"item {k} holds {c} sequences")
        if c > cap:
            raise RuntimeError(f"{c} speakers in one item; the library takes at most {cap} sequences per call")
        if total + c > cap:
            calls.append((first, k))
            first, total = k, 0
        total += c
    if first < len(counts):
        calls.append((first, len(counts)))
    return calls


def one_mixture_shape(mixes):
    """Every mixture of a batch is [M, T] and all have one shape (they share a [K,M,T] device stack): ``ValueError``
    otherwise.  Looks at shapes only.  -> (M, T), None for an empty batch."""
    shapes = [tuple(int(v) for v in np.shape(m)) for m in mixes]
    if any(len(sh) != 2 for sh in shapes):
        raise ValueError("every mixture must be [M, T]")
    if len(set(shapes)) > 1:
        raise ValueError(f"the mixtures of one batch must share M and T, got the shapes {sorted(set(shapes))}")
    return shapes[0] if shapes else None


def check_batch(mixes, sample_lists):
    """Shapes of an ``infer_batch`` call, looked at before any device work: one sample list per mixture, every mixture
    [M, T] of one shape (``one_mixture_shape``).  ``ValueError`` otherwise.  -> (M, T), (0, 0) for an empty batch."""
    if len(mixes) != len(sample_lists):
        raise ValueError(f"{len(sample_lists)} sample lists for {len(mixes)} mixtures")
    return one_mixture_shape(mixes) or (0, 0)


class SepModel(DeviceModel):
    C_PREFIX, CONFIG_C, NAME, HOT_PATH = "sep", native.SepConfigC, "SepModel", "separation network"
    param_shapes = staticmethod(sep_param_shapes)

    def __init__(self, cfg: SepConfig = SEP_FULL, state_dict=None, precision: str = "f32"):
        DeviceModel.__init__(self, cfg, precision)
        self.n_mics = cfg.n_mics
        self.max_n_speaker = cfg.max_speakers
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- device-level entry (tensors stay on the GPU) --------------------------
    def infer_device(self, mix_dev, offsets_dev):
        """mix_dev [M,T] float32 cuda, offsets_dev [S,M-1] int32 cuda (rounded) -> [S,T] float32 cuda."""
        import torch
        self._need()
        M, T = mix_dev.shape
        S = offsets_dev.shape[0]
        if S > MAX_SEQUENCES:
            raise RuntimeError(f"{S} speakers in one call; the library takes at most {MAX_SEQUENCES}")
        assert mix_dev.dtype == torch.float32 and mix_dev.is_contiguous() and mix_dev.is_cuda
        assert offsets_dev.dtype == torch.int32 and offsets_dev.is_contiguous() and offsets_dev.is_cuda
        return native.torch_ops().sep_infer(self._h.value, mix_dev, offsets_dev)

    def infer_batch_device(self, mix_stack, offsets_dev, counts):
        """``infer_device`` for K mixtures in one library call: mix_stack [K,M,T] float32 cuda, offsets_dev [N,M-1] int32
        cuda (rounded, item after item), counts [K] talkers per item (0 allowed) with N = sum(counts) <= MAX_SEQUENCES
        -> [N,T] float32 cuda.  Each item's talkers are normalised with that item's statistics and attend only to each
        other: the rows are those of ``infer_device`` item by item."""
        self._need()
        counts = [int(c) for c in counts]
        if len(counts) != mix_stack.shape[0]:
            raise RuntimeError(f"{len(counts)} counts for {mix_stack.shape[0]} mixtures")
        return native.torch_ops().sep_infer_batch(self._h.value, mix_stack, offsets_dev, counts)

    def infer_batch(self, mixes, sample_lists):
        """``infer_sample`` over a batch: mixes K x (M x T) of one shape, sample_lists K x (S_k x (M-1)) -> list of K
        float32 ndarrays [S_k, T] ((0, T) for an item with no talker).  The items go to the device whole and in order,
        in as few ``infer_batch_device`` calls as MAX_SEQUENCES allows (``pack_items``)."""
        import torch
        M, T = check_batch(mixes, sample_lists)
        offs = [rounded_offsets(sl, M - 1) for sl in sample_lists]
        counts = [o.shape[0] for o in offs]
        pack_items(counts)                                    # an item beyond the limit raises before the upload
        if sum(counts) == 0:
            return [np.empty((0, T), dtype=np.float32) for _ in mixes]
        self._need()
        stack = torch.stack([torch.as_tensor(m).to(dtype=torch.float32) for m in mixes]).to(self.device).contiguous()
        return self.infer_packed(stack, offs)

    def infer_packed(self, mix_stack, offsets):
        """mix_stack [K,M,T] float32 cuda, offsets: K rounded int32 arrays [S_k, M-1] -> K float32 ndarrays [S_k, T],
        through one ``infer_batch_device`` call per range of ``pack_items``."""
        counts = [int(o.shape[0]) for o in offsets]
        T = int(mix_stack.shape[2])
        out = []
        for first, last in pack_items(counts):
            if sum(counts[first:last]) == 0:
                out.extend(np.empty((0, T), dtype=np.float32) for _ in range(first, last))
                continue
            rows = native.to_host(self.infer_batch_device(
                mix_stack[first:last], native.to_device(np.concatenate(offsets[first:last], axis=0), mix_stack.device),
                counts[first:last]))
            pos = 0
            for c in counts[first:last]:
                out.append(rows[pos:pos + c])
                pos += c
        return out

    # ---- a recording of any length (longform.py) ----------------
    def separate_blocks(self, mix_dev, starts, T, V, offsets, row_of):
        """The blocks of a resident recording separated and stitched where they are: mix_dev [M,Ttot] float32 cuda,
        ``starts`` [K] (``longform.block_starts``), ``offsets``: K rounded int32 arrays [n_k, M-1], the talkers of every
        block, ``row_of`` [K, S] the row of track s among the rows of all blocks, block after block (-1: absent)
        -> [S, Ttot] float32 cuda.  Per range of ``pack_items`` one ``frame_blocks`` and one ``infer_batch_device``, so at
        most MAX_SEQUENCES blocks are framed at a time; then one ``stitch_blocks`` with the taper of overlap V."""
        import torch
        from . import longform
        ops = native.torch_ops()
        counts = [int(o.shape[0]) for o in offsets]
        starts = [int(a) for a in starts]
        parts = []
        for first, last in pack_items(counts):
            if sum(counts[first:last]) == 0:
                continue
            blocks = ops.frame_blocks(mix_dev, starts[first:last], int(T))
            parts.append(self.infer_batch_device(
                blocks, native.to_device(np.concatenate(offsets[first:last], axis=0), mix_dev.device), counts[first:last]))
        rows = parts[0] if len(parts) == 1 else torch.cat(parts)
        return ops.stitch_blocks(rows, native.to_device(longform.taper(T, V), mix_dev.device), starts,
                                 [int(r) for r in np.asarray(row_of).reshape(-1)], int(mix_dev.shape[1]))

    def infer_long(self, input_channels, sample_list, hop=None, block=48000) -> np.ndarray:
        """``infer_sample`` on a recording of any length: input_channels (M x Ttot), sample_list (S x (M-1)), the same
        talkers in every block -> ndarray [S, Ttot] float32.  The recording is cut into blocks of ``block`` samples every
        ``hop`` (default block - block // 8; ``longform.block_starts``, ``ValueError`` for an overlap outside
        1 .. block // 2), each block is separated like a clip of its own, and the blocks are joined by the normalised
        overlap-add of ``longform.stitch_f64``.  One upload of the mixture, one read-back of the result; framing,
        networks and stitching stay on the device (``separate_blocks``)."""
        import torch
        from . import longform
        mix = torch.as_tensor(input_channels)
        if mix.dim() != 2:
            raise ValueError("the recording must be [M, Ttot]")
        Ttot, T = int(mix.shape[1]), int(block)
        hop = T - T // 8 if hop is None else int(hop)
        starts = longform.block_starts(Ttot, T, hop)
        offs = rounded_offsets(sample_list, mix.shape[0] - 1)
        K, S = len(starts), offs.shape[0]
        pack_items([S] * K)                                   # more talkers than one call takes raise before the upload
        if S == 0:
            return np.empty((0, Ttot), dtype=np.float32)
        self._need()
        mix_d = mix.to(self.device, dtype=torch.float32).contiguous()
        return native.to_host(self.separate_blocks(mix_d, starts, T, T - hop, [offs] * K, np.arange(K * S).reshape(K, S)))

    # ---- reference call surface ---------------------------------------------------
    def infer(self, input_channels, patch_list) -> np.ndarray:
        """:492-494."""
        return self.infer_sample(input_channels, [p.sample_offset for p in patch_list])

    def infer_sample(self, input_channels, sample_list) -> np.ndarray:
        """:496-548: input_channels (M x T), sample_list (S x (M-1)) -> ndarray [S, T] float32."""
        import torch
        self._need()
        mix = torch.as_tensor(input_channels)
        offs = rounded_offsets(sample_list, mix.shape[0] - 1)
        if offs.shape[0] == 0:
            return np.empty((0, mix.shape[-1]), dtype=np.float32)
        mix_d = mix.to(self.device, dtype=torch.float32).contiguous()
        off_d = native.to_device(offs, self.device)
        return native.to_host(self.infer_device(mix_d, off_d))

    def forward(self, mix, num_speakers):
        """Network.forward (:418-490): mix [B, S*M, t] already normalised, num_speakers [B,1]
        -> device tensor [B, max(max(S), max_speakers), t].  Items may hold different numbers of speakers: like the
        reference (speakers_to_batches / batches_to_speakers, :236-268) only the first num_speakers[b] blocks of M
        channels of item b are read, a missing speaker takes part in the inter-speaker attention as a zero sequence,
        its output row is the bare output_decoder bias, and the stack is as wide as the largest count."""
        import torch
        self._need()
        ns = np.asarray(torch.as_tensor(num_speakers).cpu()).reshape(-1).astype(np.int64)
        mix = torch.as_tensor(mix).to(self.device, dtype=torch.float32).contiguous()
        B, SM, t = mix.shape
        if ns.shape[0] != B or B < 1:
            raise RuntimeError(f"num_speakers holds {ns.shape[0]} entries for {B} batch items")
        S = int(ns.max())
        if ns.min() < 1 or SM % self.n_mics != 0 or SM < S * self.n_mics:
            raise RuntimeError(f"mix has {SM} channels, expected at least max(num_speakers)*n_mics = {S * self.n_mics}")
        if B * S > MAX_SEQUENCES:
            raise RuntimeError(f"{B * S} sequences in one call; the library takes at most {MAX_SEQUENCES}")
        if np.all(ns == S) and SM == S * self.n_mics:
            return native.torch_ops().sep_forward(self._h.value, mix, S, self.n_mics, self.max_n_speaker)
        if SM != S * self.n_mics:
            mix = mix[:, :S * self.n_mics].contiguous()       # blocks beyond the largest count are never read (:244)
        return native.torch_ops().sep_forward_counts(self._h.value, mix, [int(v) for v in ns], self.n_mics, self.max_n_speaker)

    __call__ = forward
