"""Host-side mirror of the reference's spot-model call surface over libasw_hip.so.

``SpotModel`` keeps the names, argument meaning and return types of
``DataParallelSpotModel.shift_and_sep`` (sep/training/JointModel/network.py:27-104) and
``Network.forward`` (sep/training/SpeakerLocalization/network.py:363-405); all
arithmetic runs in the HIP library, reached through the PyTorch-ROCm custom ops
``torch.ops.asw.*`` (csrc/torch_ops.cpp, thin adapters over the C ABI).  PyTorch is used only
for device memory and streams.  ``shift_and_score`` is the additive energies-only fast path:
waveforms stay on the GPU, two doubles per candidate come back.
"""
import numpy as np

from . import native
from .config import FULL, SpotConfig, spot_param_shapes
from .device_model import DeviceModel
from .scorer import DeviceScorer


def offsets_from_patches(patch_list, n_pairs: int = None) -> np.ndarray:
    """round(sample_offset) per candidate as int32 [N, M-1]
    (JointModel/network.py:81-82: the offsets pass through a float32 torch.Tensor before
    torch.round, which is round-half-even == np.rint on the float32 value).  ``patch_list``: patches or rows of
    offsets; ``n_pairs``: the M-1 they must have (None: whatever they have)."""
    if len(patch_list) == 0:
        return np.zeros((0, n_pairs or 0), dtype=np.int32)
    offs = np.stack([np.asarray(getattr(p, "sample_offset", p), dtype=np.float64) for p in patch_list])
    if n_pairs is not None and offs.shape[1] != n_pairs:
        raise RuntimeError(f"candidate has {offs.shape[1]} offsets, mixture has {n_pairs + 1} channels")
    return np.rint(offs.astype(np.float32)).astype(np.int32)


class SpotModel(DeviceModel, DeviceScorer):
    """The spot network's handle (``DeviceModel``: weights, ``to``, precision, taps) with the calls that need the
    network; the device helpers that need none -- SI-SDR, segments, the decision kernels -- are ``DeviceScorer``'s."""
    C_PREFIX, CONFIG_C, NAME, HOT_PATH = "spot", native.SpotConfigC, "SpotModel", "spot hot path"
    param_shapes = staticmethod(spot_param_shapes)

    def __init__(self, cfg: SpotConfig = FULL, state_dict=None, batch_size: int = 32, precision: str = "f32",
                 lanes: int = 1):
        """precision: "f32" = exact fp32 MFMA; "f16x3" = split-operand half MFMA with fp32
        accumulation (~21-bit operands, 5.3x the f32 matrix rate), see csrc/convgemm.hip (and pipegemm.hip, resconv.hip);
        "f16x3_safe" = f16x3 wherever a GEMM reads a normalised tensor, exact f32 (and a per-frame scale in the
        one-launch mask path) where it reads an un-normalised one, so that no magnitude can saturate the fp16 split
        (csrc/model_common.h, Trunk::site)."""
        DeviceModel.__init__(self, cfg, precision)
        self.batch_size = batch_size
        self.lanes = int(lanes)             # 2: consecutive internal batches on two HIP streams (asw_spot_set_lanes)
        self.last_waveforms = None          # device tensor [N,T] of the latest shift_and_score
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def _reload_context(self):
        """SpotModel's own: the handle's device if one is set, else no context at all."""
        import contextlib
        import torch
        return torch.cuda.device(self.device) if self.device is not None else contextlib.nullcontext()

    def _configure(self):
        native.check(self._c("set_batch")(self._h, int(self.batch_size)))
        DeviceModel._configure(self)
        native.check(self._c("set_lanes")(self._h, self.lanes))

    def set_lanes(self, lanes: int):
        self.lanes = int(lanes)
        if self._h is not None:
            native.check(native.lib().asw_spot_set_lanes(self._h, self.lanes))

    def set_batch_size(self, b: int):
        self.batch_size = int(b)
        if self._h is not None:
            native.check(native.lib().asw_spot_set_batch(self._h, int(b)))

    # ---- device-level entry (tensors stay on the GPU) --------------------------
    def shift_and_sep_device(self, mix_dev, offsets_dev, strict: int = 0, want_wave: bool = True,
                             want_energy: bool = False, window: int = 12000, circular: bool = True):
        """mix_dev [M,T] float32 cuda, offsets_dev [N,M-1] int32 cuda ->
        (wave [N,T] float32 cuda | None, energy [N,2] float64 cuda | None)."""
        import torch
        self._need()
        M, T = mix_dev.shape
        N = offsets_dev.shape[0]
        assert mix_dev.dtype == torch.float32 and mix_dev.is_contiguous() and mix_dev.is_cuda
        assert offsets_dev.dtype == torch.int32 and offsets_dev.is_contiguous() and offsets_dev.is_cuda
        # torch.ops.asw.spot_shift_and_sep: runs on the tensors' device and torch's current stream
        wave, en = native.torch_ops().spot_shift_and_sep(self._h.value, mix_dev, offsets_dev, int(strict), bool(circular),
                                                         bool(want_wave), bool(want_energy), int(window))
        return (wave if want_wave else None), (en if want_energy else None)

    def shift_and_sep_device_multi(self, mix_stack, offsets_dev, mix_index_dev, strict: int = 0, want_wave: bool = True,
                                   want_energy: bool = False, window: int = 12000, circular: bool = True):
        """The same call over candidates of several mixtures (torch.ops.asw.spot_shift_and_sep_multi):
        mix_stack [K,M,T] float32 cuda, offsets_dev [N,M-1] int32, mix_index_dev [N] int32 with values in [0,K)
        (the caller builds it on the host and guarantees the range)."""
        import torch
        self._need()
        assert mix_stack.dim() == 3 and mix_stack.dtype == torch.float32 and mix_stack.is_contiguous() and mix_stack.is_cuda
        assert offsets_dev.dtype == torch.int32 and offsets_dev.is_contiguous() and offsets_dev.is_cuda
        assert mix_index_dev.dtype == torch.int32 and mix_index_dev.is_contiguous() and mix_index_dev.is_cuda
        wave, en = native.torch_ops().spot_shift_and_sep_multi(self._h.value, mix_stack, offsets_dev, mix_index_dev,
                                                               int(strict), bool(circular), bool(want_wave),
                                                               bool(want_energy), int(window))
        return (wave if want_wave else None), (en if want_energy else None)

    # ---- reference call surface ---------------------------------------------------
    def shift_and_sep(self, input_channels, patch_list, Strict: int = 0, save_input: bool = False) -> np.ndarray:
        """Drop-in for DataParallelSpotModel.shift_and_sep: returns ndarray [N,T] float32."""
        import torch
        self._need()
        if save_input:
            raise RuntimeError("save_input=True is a debugging path of the reference that materialises every "
                               "shifted mixture; it is not provided (the shifted tensor never exists here)")
        mix = torch.as_tensor(input_channels)
        T = mix.shape[-1]
        if len(patch_list) == 0:
            return np.empty((0, T), dtype=np.float32)
        offs = offsets_from_patches(patch_list, mix.shape[0] - 1)
        mix_d = mix.to(self.device, dtype=torch.float32).contiguous()
        off_d = torch.from_numpy(offs).to(self.device)
        wave, _ = self.shift_and_sep_device(mix_d, off_d, Strict, want_wave=True)
        return native.to_host(wave)

    def shift_and_score(self, input_channels, patch_list, Strict: int = 0, window: int = 12000,
                        keep_waveforms: bool = True) -> np.ndarray:
        """Energies-only fast path: ndarray [N,2] float64 = (power, power2) of every
        mean-removed candidate output (local_utils_3d.py:349-354 / Mic_Array.py:290-295)."""
        import torch
        self._need()
        mix = torch.as_tensor(input_channels)
        if len(patch_list) == 0:
            self.last_waveforms = None
            return np.empty((0, 2), dtype=np.float64)
        offs = offsets_from_patches(patch_list, mix.shape[0] - 1)
        mix_d = mix.to(self.device, dtype=torch.float32).contiguous()
        off_d = torch.from_numpy(offs).to(self.device)
        wave, en = self.shift_and_sep_device(mix_d, off_d, Strict, want_wave=keep_waveforms, want_energy=True,
                                             window=window)
        self.last_waveforms = wave
        return en.cpu().numpy()

    def shift_and_sep_resident(self, input_channels, patch_list, Strict: int = 0, window: int = 12000,
                               device_energies: bool = False):
        """Device-resident variant for the fine stage: returns (waves, energies) where ``waves``
        is a CUDA tensor [N,T] of the MEAN-REMOVED candidate outputs (sep/Mic_Array.py:291) that
        stays on the GPU, and ``energies`` the host ndarray [N,2] = (power, power2).  Only the
        energies (and later the few cluster heads) cross PCIe.  With ``device_energies`` the
        energies stay on the GPU too and nothing in the call waits for the device (the offsets go
        up through pinned memory), so the caller can overlap host work with it."""
        import torch
        self._need()
        mix = torch.as_tensor(input_channels)
        offs = offsets_from_patches(patch_list, mix.shape[0] - 1)
        mix_d = mix.to(self.device, dtype=torch.float32).contiguous()
        if device_energies:
            off_d = torch.from_numpy(offs).pin_memory().to(self.device, non_blocking=True)
        else:
            off_d = torch.from_numpy(offs).to(self.device)
        wave, en = self.shift_and_sep_device(mix_d, off_d, Strict, want_wave=True, want_energy=True, window=window)
        native.torch_ops().center_rows_(wave)
        return wave, (en if device_energies else en.cpu().numpy())

    def score_offsets(self, input_channels, offsets, Strict: int = 0, window: int = 12000):
        """``shift_and_score`` on a table of offsets instead of a patch list, with the result left where it was written:
        ``offsets`` int32 [N, M-1], an ndarray or a tensor on the model's device -> the device tensor [N,2] float64 =
        (power, power2).  A host table goes up through pinned memory; nothing comes back and nothing waits for the
        device."""
        import torch
        self._need()
        mix = torch.as_tensor(input_channels)
        mix_d = mix.to(self.device, dtype=torch.float32).contiguous()
        if isinstance(offsets, torch.Tensor):
            off_d = offsets.to(self.device, dtype=torch.int32).contiguous()
        else:
            off_d = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int32)).pin_memory().to(self.device, non_blocking=True)
        if off_d.dim() != 2 or off_d.shape[1] != mix_d.shape[0] - 1:
            raise RuntimeError(f"offsets of shape {tuple(off_d.shape)} do not fit a mixture of {mix_d.shape[0]} channels")
        if off_d.shape[0] == 0:
            return torch.empty((0, 2), dtype=torch.float64, device=self.device)
        _wave, en = self.shift_and_sep_device(mix_d, off_d, Strict, want_wave=False, want_energy=True, window=window)
        return en

    def forward(self, mix, window_embedding):
        """Network.forward: mix [B,M,t] (already normalised), window_embedding [B,2] -> [B,1,t]
        (device tensor).  Rows are grouped by identical embedding because the window gate
        is folded into the convolution weights."""
        import torch
        self._need()
        mix = torch.as_tensor(mix).to(self.device, dtype=torch.float32).contiguous()
        wemb = torch.as_tensor(window_embedding, dtype=torch.float32).cpu().numpy().reshape(mix.shape[0], 2)
        B, M, t = mix.shape
        out = torch.empty((B, 1, t), dtype=torch.float32, device=self.device)
        keys = {}
        for i, row in enumerate(map(tuple, wemb)):
            keys.setdefault(row, []).append(i)
        ops = native.torch_ops()
        for row, idx in keys.items():
            whole = len(idx) == B
            y = ops.spot_forward(self._h.value, mix if whole else mix[idx].contiguous(), float(row[0]), float(row[1]))
            if whole:
                return y.view(B, 1, t)
            out.view(B, t)[idx] = y
        return out

    __call__ = forward

    def set_fused_mask(self, on: bool = True):
        """f16x3 mode: run the mask path (bypass, mask encoder, product, decoder taps) as one launch
        (default) or as three GEMMs (the "latent" tap exists only then)."""
        self._need()
        native.check(native.lib().asw_spot_set_fused_mask(self._h, int(bool(on))))
        return self

    def set_source_stack(self, on: bool = True):
        """f16x3 mode: shift_and_sep folds the 1x1 preproc into encoder block 0's first residual layer (default;
        the "preproc" tap does not exist then) or runs the separate preproc pass (asw_spot_set_source_stack)."""
        self._need()
        native.check(native.lib().asw_spot_set_source_stack(self._h, int(bool(on))))
        return self

    def set_up_fusion(self, on: bool = True):
        """f16x3 mode: in shift_and_sep the residual stack in front of a 64 -> 64 channel decoder block applies that
        block's upsampling itself (default; the tap of the block in front does not exist then) or leaves it to the
        separate GEMM launch (asw_spot_set_up_fusion)."""
        self._need()
        native.check(native.lib().asw_spot_set_up_fusion(self._h, int(bool(on))))
        return self
