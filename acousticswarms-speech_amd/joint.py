"""Pipeline driver with the call surface of the reference ``JointModel``
(sep/training/JointModel/network.py:106-215): ``setup`` / ``forward`` /
``localize_by_separation`` / ``separate_by_localization`` and the five stage timers
``times[0..4]`` = [SRP, coarse, fine, clustering, joint separation] seconds.

Unlike the reference's timers (host ``time.time()`` with no device synchronisation,
:143-148) each stage boundary here synchronises the device, so the numbers are true
stage latencies.  ``sep_model`` is the joint separation network (``sep.SepModel``, the HIP
implementation of sep/training/SpeakerSeparation/network.py) or any object with
``infer(mix, patches)``; with ``sep_model=None`` the separation stage is skipped, ``audio`` is
None and ``times[4]`` stays 0 (callers must then report a localize-only latency).
"""
import collections
import threading
import time

import numpy as np

from .longform import LINK_RADIUS
from .mic_array import MicArray, run_search
from .modes import MODE_NAMES, check_modes


def _sync():
    """Stage boundary: every stream of the device drained, then one event round trip on the current stream.
    The round trip is not decoration.  After hipDeviceSynchronize / hipStreamSynchronize alone the ROCm 7.2
    runtime intermittently (about every second forward) starts the FIRST command of the next stage 20-25 ms
    late: the whole stage is enqueued within a few ms but nothing executes until that long into the stage's
    final blocking copy (rocprofv3 --hip-trace --kernel-trace; the separation stage read 23 or 45-60 ms,
    tests/micro/e2e_stats.py).  With a hipEventRecord + hipEventSynchronize after the drain the next
    submission is dispatched at once: 12 of 12 forwards at 23 ms.  (Event record without the wait, stream
    synchronize, or no synchronisation at all: the late start stays.)"""
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize()
            ev = torch.cuda.Event()
            ev.record()
            ev.synchronize()
    except ImportError:          # pragma: no cover
        pass


GEOMETRY_CACHE_SIZE = 8        # arrays kept by JointModel.mic_array_for (a 7-mic bench array: about 65 MB of tables)


def config_key(mic_positions, speaker_range, prone_method="SRP", geometry="host", segments="host", clustering="host",
               global_clustering="host", coarse="host"):
    """The configuration string of the reference's ``setup`` (:125-131), extended by the pruning method and by every
    mode (``modes.MODE_NAMES``, in that order) that is not at its default."""
    key = '~'.join([f"{x:.05f}" for x in np.asarray(mic_positions).flatten()]) \
        + '|' + '~'.join([f"{x:.05f}" for x in speaker_range])
    if prone_method != "SRP":
        key += '|' + str(prone_method)
    for name, value in zip(MODE_NAMES, (geometry, segments, clustering, global_clustering, coarse)):
        if value != "host":
            key += '|' + name + '=' + str(value)
    return key


class _Pending(object):
    """A geometry another thread is building (JointModel.mic_array_for)."""
    __slots__ = ("done", "value", "error")

    def __init__(self):
        self.done, self.value, self.error = threading.Event(), None, None


class JointModel(object):
    def __init__(self, spot_model, sep_model=None, device=None, geometry="host", segments="host", clustering="host",
                 global_clustering="host", coarse="host"):
        """The five modes (``modes.MODE_NAMES``; ``MicArray.__init__`` describes them) are the defaults of ``setup``'s
        arguments of these names and the modes of the per-mixture arrays of ``mic_array_for``.  The rule that needs a
        ``prone_method`` (``coarse="device"``) is checked at ``setup`` / ``mic_array_for``, where one is known."""
        for name, value in zip(MODE_NAMES, check_modes(geometry, segments, clustering, global_clustering, coarse)):
            setattr(self, name, value)
        self.spot_model = spot_model
        self.sep_model = sep_model
        self.device = device
        self._geometry_cache = collections.OrderedDict()      # config key -> MicArray | _Pending, least recent first
        self._geometry_lock = threading.Lock()
        self.geometry_stats = {"builds": 0, "hits": 0}
        self.times = [0, 0, 0, 0, 0]
        self.previous_config = None
        self.Mic_processor = None
        self._mix_dev = self._mix_src = None

    def setup(self, mic_positions, speaker_range, cached=False, cached_folder=None, prone_method="SRP", geometry=None,
              segments=None, clustering=None, global_clustering=None, coarse=None):
        """(Re)build the geometry tables unless the configuration is unchanged (:125-137).
        One-off per geometry and excluded from latency, as the reference's README notes.
        ``prone_method`` picks the stage-1 pruning map ("SRP", "MUSIC" or "TOPS"; "DENSE": no pruner, the whole
        coarse TDoA lattice of the array) and is part of the configuration, and so is each of the five modes
        ("host" | "device", default: the model's; ``MicArray.__init__`` describes them)."""
        modes = self._modes(geometry, segments, clustering, global_clustering, coarse)
        key = config_key(mic_positions, speaker_range, prone_method, **modes)
        if key == self.previous_config:
            print("reuse the previous recycle!")
            return
        import gc
        gc.unfreeze()                       # a previous geometry may go now
        self.Mic_processor = MicArray(mic_positions, Spk_Range=speaker_range, Prone_method=prone_method,
                                      device=self.device, **modes)
        self.previous_config = key
        # The geometry tables are tens of thousands of small arrays and lists that live as long as
        # this configuration.  Left in the collector's oldest generation they make every full
        # collection of the interpreter a 50 ms pause that lands at random inside a forward()
        # (measured: 22-66 ms on the first statement after the search).  Move them to the permanent
        # generation: later collections only look at what a forward() itself allocates.
        gc.collect()
        gc.freeze()

    def _modes(self, *given):
        """The five modes as the keywords of ``config_key`` / ``MicArray``: the model's, or ``given`` (in the order of
        ``MODE_NAMES``) where that is not None."""
        values = [getattr(self, name) if value is None else value
                  for name, value in zip(MODE_NAMES, given or [None] * len(MODE_NAMES))]
        return dict(zip(MODE_NAMES, check_modes(*values)))

    def mic_array_for(self, mic_positions, speaker_range, prone_method="SRP"):
        """The ``MicArray`` of one mixture's own geometry (batch path, ``geometries=``), built in the model's
        ``geometry`` mode and kept in a small LRU keyed like ``previous_config``: an array that repeats within a
        batch is built once, and two searches asking for the same array at the same time share one build (the
        second waits for the first).  Thread-safe; ``geometry_stats`` counts builds and hits.

        Unlike ``setup`` this does not run ``gc.collect()`` / ``gc.freeze()``: that pair walks the whole heap
        (tens of ms) and a per-mixture array does not live long enough to be worth moving to the permanent
        generation.  Instead the batch raises the collector's oldest-generation threshold while it runs
        (``batching.no_full_collections``), so no full collection lands inside a search, and an evicted array is
        released by reference counting alone -- its tables hold no reference cycle."""
        modes = self._modes()
        key = config_key(mic_positions, speaker_range, prone_method, **modes)
        with self._geometry_lock:
            hit = self._geometry_cache.get(key)
            if hit is None:
                pending = _Pending()
                self._geometry_cache[key] = pending
            else:
                self._geometry_cache.move_to_end(key)
        if hit is not None:
            if isinstance(hit, _Pending):
                hit.done.wait()
                if hit.error is not None:
                    raise hit.error
                hit = hit.value
            with self._geometry_lock:
                self.geometry_stats["hits"] += 1
            return hit
        try:
            mp = MicArray(np.asarray(mic_positions), Spk_Range=speaker_range, Prone_method=prone_method,
                          device=self.device, **modes)
        except BaseException as exc:
            with self._geometry_lock:
                self._geometry_cache.pop(key, None)
            pending.error = exc
            pending.done.set()
            raise
        with self._geometry_lock:
            self.geometry_stats["builds"] += 1
            self._geometry_cache[key] = mp
            ready = [k for k, v in self._geometry_cache.items() if not isinstance(v, _Pending)]
            for k in ready[:max(0, len(ready) - GEOMETRY_CACHE_SIZE)]:
                del self._geometry_cache[k]
        pending.value = mp
        pending.done.set()
        return mp

    def use_geometry(self, mic_positions, speaker_range):
        """Make the cached array of this geometry (``mic_array_for``) the one ``forward`` searches with: the plain
        per-mixture loop of ``shard.localize_batch(..., geometries=...)``."""
        method = self.Mic_processor.Prone_method if self.Mic_processor is not None else "SRP"
        self.Mic_processor = self.mic_array_for(mic_positions, speaker_range, method)
        self.previous_config = config_key(mic_positions, speaker_range, method, **self._modes())

    def forward(self, mix_data):
        """-> (patches, audio_loc, audio, SRP_drop, stage1_drop, spot_times) (:142-149)."""
        self.times = [0, 0, 0, 0, 0]
        patches, audio_loc, SRP_drop, stage1_drop, spot_times = self.localize_by_separation(mix_data)
        _sync()
        t0 = time.time()
        audio = self.separate_by_localization(mix_data, patches)
        _sync()
        self.times[4] = time.time() - t0
        self._mix_dev = self._mix_src = None              # the resident copy does not outlive the forward
        return patches, audio_loc, audio, SRP_drop, stage1_drop, spot_times

    __call__ = forward

    def _timed(self, slot, fn, *args):
        _sync()
        t0 = time.time()
        out = fn(*args)
        _sync()
        self.times[slot] = time.time() - t0
        return out

    def localize_by_separation(self, mix_data):
        """The four search stages with the reference's empty-result early returns (:151-199): ``mic_array.run_search``
        under this model's device-synchronised timers, its one upload of the mixture and the reference's printed lines."""
        assert self.previous_config is not None, \
            "Microphone positions and spk range were not provided, did you forget to call .setup()?"
        mp = self.Mic_processor
        # One upload of the mixture per forward, inside the first timed stage: the HIP models take
        # the resident copy (a host tensor would be copied again by every stage -- and a pageable
        # H2D right after the fine stage was measured at 29 ms for these 1.3 MB).  Any other
        # duck-typed model keeps receiving the caller's tensor.
        self._mix_dev = self._mix_src = None

        def srp_stage(m):
            self._mix_dev = self._resident(m)
            self._mix_src = m                             # the resident copy stands for THIS object only
            return mp.Apply_SRP_PHAT(m)

        def stage_mix():                                  # the scoring stages of a HIP model read the resident copy
            resident = self._takes_resident(self.spot_model) and self._mix_dev is not None
            return self._mix_dev if resident else mix_data
        patch_final, audio_final, spot_times, empty = run_search(mp, self.spot_model, self._timed, mix_data,
                                                                 stage_mix, srp_stage)
        if empty is not None:
            print(f"No spk picked in {empty}")
            return [], [], 0, 0, 0
        return patch_final, np.array(audio_final), 0, 0, spot_times

    @staticmethod
    def _takes_resident(model):
        """HIP models of this package (SpotModel / SepModel) accept a device-resident mixture."""
        dev = getattr(model, "device", None)
        return getattr(dev, "type", None) == "cuda" and (hasattr(model, "shift_and_sep_device") or hasattr(model, "infer_device"))

    def _resident(self, mix_data):
        for m in (self.spot_model, self.sep_model):
            if m is not None and self._takes_resident(m):
                import torch
                return torch.as_tensor(mix_data).to(m.device, dtype=torch.float32).contiguous()
        return None

    def separate_by_localization(self, mix_data, target_patches):
        if len(target_patches) == 0 or self.sep_model is None:
            return None
        # the resident copy uploaded by localize_by_separation() is reused only for the very object it was made
        # from (or for itself): a different mixture of the same shape must not be swapped for the cached one
        cached = getattr(self, "_mix_dev", None)
        if self._takes_resident(self.sep_model) and cached is not None \
                and (mix_data is getattr(self, "_mix_src", None) or mix_data is cached):
            mix_data = cached
        return self.sep_model.infer(mix_data, [p[0] for p in target_patches])

    def separate_by_localization_by_sample(self, mix_data, sample_lists):
        """:206-209: the separation stage from sample offsets instead of patches."""
        if len(sample_lists) == 0:
            return None
        return self.sep_model.infer_sample(mix_data, sample_lists)

    def separate_batch(self, mixes, patch_lists):
        """The separation stage of a batch: ``patch_lists[k]`` are the final patches of mixture k as ``forward`` returns
        them (tuples whose first entry is the patch).  -> list of float32 ndarrays [S_k, T], (0, T) for a mixture with
        no talker (``SepModel.infer_batch``: the mixtures of one shape, packed into as few device calls as fit)."""
        if self.sep_model is None:
            raise RuntimeError("separate_batch needs a separation model (sep_model=None)")
        return self.sep_model.infer_batch(mixes, [[p[0].sample_offset for p in patches] for patches in patch_lists])

    def forward_long(self, mix_data, block=48000, hop=None, localize="every", link_radius=LINK_RADIUS):
        """Localise and separate a recording of any length on the array of ``setup()``: mix_data [M, Ttot] is cut into
        blocks of ``block`` samples every ``hop`` (default block - block // 8; ``longform.block_starts``), the blocks
        are searched, every block separates its talkers, and the tracks are joined by the normalised overlap-add of
        ``longform.stitch_f64`` on the device (``SepModel.separate_blocks``: one upload, one read-back).

        ``localize="every"``: every block is searched (``shard.localize_batch``, the blocks sharing their network
        launches), the detections are linked into tracks by position (``longform.link_tracks``, ``link_radius`` metres),
        and a block separates the talkers found in it, at the sample offsets
        ``forward`` would separate them at; a track fades out over the seam into a block it was not found in.
        ``localize="first"``: block 0 alone is searched and its talkers are separated in every block.

        -> dict: ``audio`` float32 [n_tracks, Ttot]; ``present`` bool [n_tracks, K]; ``detection`` int64 [n_tracks, K],
        the talker of block k that is the track (its row in that block's search result; -1 when absent);
        ``positions``: {"per_block": float64 [n_tracks, K, 3], the centre in every block the track is present in (NaN
        elsewhere; with "first", block 0's centre throughout), "mean": [n_tracks, 3]}; ``starts`` int64 [K]; ``blocks``:
        the search results, one dict per searched block as ``localize_batch(..., details=True)`` returns them.

        Needs a HIP separation model and a single rank (``RuntimeError`` otherwise, as ``separate=True``)."""
        import torch
        from . import longform
        from .batching import result_record
        from .sep import rounded_offsets
        if localize not in ("every", "first"):
            raise ValueError(f'localize must be "every" or "first", got {localize!r}')
        if self.sep_model is None or not hasattr(self.sep_model, "separate_blocks"):
            raise RuntimeError("forward_long needs a separation model (JointModel(sep_model=None))")
        import torch.distributed as dist
        if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) \
                or getattr(self.spot_model, "world", 1) > 1:
            raise RuntimeError("forward_long runs on one rank only: the audio is not gathered across ranks")
        assert self.previous_config is not None, \
            "Microphone positions and spk range were not provided, did you forget to call .setup()?"
        mix = torch.as_tensor(mix_data).to(dtype=torch.float32)
        if mix.dim() != 2:
            raise ValueError("the recording must be [M, Ttot]")
        (M, Ttot), T = (int(v) for v in mix.shape), int(block)
        hop = T - T // 8 if hop is None else int(hop)
        starts = longform.block_starts(Ttot, T, hop)
        K = len(starts)
        host = mix.cpu().numpy()
        if localize == "first":
            first = torch.from_numpy(longform.frame_f64(host, starts[:1], T, np.float32)[0])
            self.times = [0, 0, 0, 0, 0]
            patches, _audio_loc, _d0, _d1, spot_times = self.localize_by_separation(first)
            self._mix_dev = self._mix_src = None
            results = [result_record(patches, spot_times, list(self.times), True, (M, T))]
            n = len(patches)
            offsets = [rounded_offsets(list(results[0]["offsets"]), M - 1)] * K
            det_of = np.tile(np.arange(n, dtype=np.int64), (K, 1))
            per_block = np.repeat(results[0]["centres"].reshape(n, 1, 3), K, axis=1)
        else:
            from .shard import localize_batch
            frames = longform.frame_f64(host, starts, T, np.float32)
            results = localize_batch(self, [torch.from_numpy(f) for f in frames], details=True)
            offsets = [rounded_offsets(list(r["offsets"]), M - 1) for r in results]
            det_of, per_block = longform.link_tracks([r["centres"] for r in results], float(link_radius))
        n_tracks = det_of.shape[1]
        if n_tracks == 0:
            audio = np.empty((0, Ttot), dtype=np.float32)
        else:
            from . import native
            sep = self.sep_model
            audio = native.to_host(sep.separate_blocks(mix.to(sep.device).contiguous(), starts, T, T - hop, offsets,
                                                       longform.rows_of(det_of, [o.shape[0] for o in offsets])))
        return {"audio": audio, "present": (det_of >= 0).T, "detection": det_of.T.copy(),
                "positions": {"per_block": per_block, "mean": np.nanmean(per_block, axis=1).reshape(n_tracks, 3)},
                "starts": starts, "blocks": results}

    def to(self, device=None):
        if device is not None:
            self.device = device
            if hasattr(self.spot_model, "to"):
                self.spot_model.to(device)
            if self.sep_model is not None and hasattr(self.sep_model, "to"):
                self.sep_model.to(device)
        return self
