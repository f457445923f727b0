"""The lifecycle the two network handles of libasw_hip.so share: ``spot.SpotModel`` and ``sep.SepModel`` are views of
``DeviceModel``.  The base owns the precision table, the cleaning and the refusals of a state dict, the upload, ``to``
(destroy, create, configure, upload under the handle's device), ``set_precision``, ``get_tap`` and the two
"not ready" refusals.  A subclass states its C prefix (``asw_<prefix>_create`` ...), its config struct, its
parameter-shape function, its words for the messages and, where it has more than a precision, its setters after
``create`` (``_configure``)."""
from collections import OrderedDict
from ctypes import byref, c_size_t, c_void_p

import numpy as np

from . import native


class DeviceModel:
    PRECISIONS = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3_safe": 3}

    # what a subclass states
    C_PREFIX = None             # "spot" | "sep": the handle's functions are asw_<prefix>_<name>
    CONFIG_C = None             # native.SpotConfigC | native.SepConfigC
    NAME = None                 # the class name as the messages spell it
    HOT_PATH = None             # "no HIP device visible: the <HOT_PATH> has no CPU fallback"
    param_shapes = None         # staticmethod: cfg -> [(name, shape), ...] in the reference's state-dict order

    def __init__(self, cfg, precision):
        if precision not in self.PRECISIONS:
            raise RuntimeError(f"precision must be one of {list(self.PRECISIONS)}")
        self.cfg = cfg
        self.precision = precision
        self.device = None
        self._h = None
        self._sd = None

    def _c(self, name):
        return getattr(native.lib(), f"asw_{self.C_PREFIX}_{name}")

    # ---- weights -------------------------------------------------------------
    def load_state_dict(self, sd, strict: bool = True):
        """Reference-format state dict (numpy arrays or torch tensors), strict by default."""
        want = OrderedDict(self.param_shapes(self.cfg))
        clean = OrderedDict()
        for k, v in sd.items():
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            clean[k] = np.ascontiguousarray(a, dtype=np.float32)
        missing = [k for k in want if k not in clean]
        extra = [k for k in clean if k not in want]
        if strict and (missing or extra):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:3]} unexpected {extra[:3]}")
        for k, shp in want.items():
            if k in clean and tuple(clean[k].shape) != tuple(shp):
                raise RuntimeError(f"size mismatch for {k}: {tuple(clean[k].shape)} vs {tuple(shp)}")
        self._sd = clean
        if self._h is not None:
            with self._reload_context():
                self._upload()
        return self

    def _reload_context(self):
        """The device context ``load_state_dict`` uploads under when the handle exists already.  The two classes differ
        here and stay different: this is SepModel's, always the handle's device; SpotModel overrides it."""
        import torch
        return torch.cuda.device(self.device)

    def _upload(self):
        set_param = self._c("set_param")
        for k, a in self._sd.items():
            native.check(set_param(self._h, k.encode(), c_void_p(a.ctypes.data), a.size))
        native.check(self._c("finalize")(self._h))

    def to(self, device=None):
        """Create the device-resident model (weights uploaded once; C1 of SURVEY.md §2.2)."""
        import torch
        if device is None:
            return self
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"{self.NAME} runs only on an MI355X (device 'cuda'); there is no CPU path")
        if not torch.cuda.is_available():
            raise RuntimeError(f"no HIP device visible: the {self.HOT_PATH} has no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(device):            # the handle lives on this device; the process default is untouched
            if self._h is not None:
                self._c("destroy")(self._h)
                self._h = None
            h = c_void_p()
            cc = self.CONFIG_C.from_config(self.cfg)
            native.check(self._c("create")(byref(cc), byref(h)))
            self._h = h
            self._configure()
            self.device = device
            if self._sd is not None:
                self._upload()
        return self

    def _configure(self):
        """The setters after ``create``, under the new handle's device."""
        native.check(self._c("set_precision")(self._h, self.PRECISIONS[self.precision]))

    def eval(self):
        return self

    def set_precision(self, precision: str):
        if precision not in self.PRECISIONS:
            raise RuntimeError(f"precision must be one of {list(self.PRECISIONS)}")
        self.precision = precision
        if self._h is not None:
            native.check(self._c("set_precision")(self._h, self.PRECISIONS[precision]))

    def __del__(self):
        try:
            if self._h is not None:
                self._c("destroy")(self._h)
        except Exception:
            pass

    def _need(self):
        if self._h is None:
            raise RuntimeError(f"{self.NAME}.to('cuda') must be called before inference")
        if self._sd is None:
            raise RuntimeError(f"{self.NAME} has no weights: call load_state_dict()")

    def get_tap(self, name: str, shape=None):
        """Intermediate activation of the last call (channels-last), for parity tests."""
        import torch
        n = c_size_t()
        tap = self._c("get_tap")
        native.check(tap(self._h, name.encode(), None, 0, byref(n), None))
        buf = torch.empty((n.value,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            native.check(tap(self._h, name.encode(), native.ptr(buf), n.value, byref(n), native.current_stream()))
        return buf if shape is None else buf.view(*shape)
