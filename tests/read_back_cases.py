"""The tensors ``native.read_back`` is checked on, shared by the host and the GPU test: the four dtypes of the search's
read-backs at 0, 1, 3 and 5 elements in an order that puts the later pieces at byte offsets that are no multiple of 8
(or of 4), a 2-D shape, a non-contiguous column, a 0-d tensor, and NaN, +-Inf and -0.0 among the float64 values."""
import numpy as np
import torch

SPECIAL = [np.nan, np.inf, -np.inf, -0.0, 0.0]


def make_cases(device="cpu"):
    rng = np.random.default_rng(11)
    wide = torch.from_numpy(rng.standard_normal((4, 3)))
    cpu = [
        torch.arange(5, dtype=torch.uint8),                                  # the next piece starts at byte 5
        torch.tensor(SPECIAL[:3], dtype=torch.float64),
        torch.zeros(0, dtype=torch.int32),
        torch.tensor([7], dtype=torch.uint8),                                # ... and the next at byte 30
        torch.arange(-3, 3, dtype=torch.int32).reshape(2, 3),
        torch.from_numpy(rng.standard_normal(5).astype(np.float32)),
        torch.tensor([1, 2, 3], dtype=torch.uint8),
        torch.tensor(SPECIAL, dtype=torch.float64),
        torch.tensor([-2 ** 31], dtype=torch.int32),
        torch.tensor([np.nan, -0.0, np.inf], dtype=torch.float32),
        torch.zeros(0, dtype=torch.float64),
        torch.tensor(2.5, dtype=torch.float64),                              # 0-d
        torch.tensor([-1.5], dtype=torch.float64),
        torch.zeros((0, 2), dtype=torch.float64),
        torch.zeros(0, dtype=torch.uint8),
        torch.zeros(0, dtype=torch.float32),
        torch.tensor([3.25], dtype=torch.float32),
        torch.arange(3, dtype=torch.int32),
        torch.arange(5, dtype=torch.int32),
    ]
    cases = [t.to(device) for t in cpu]
    column = wide.to(device)[:, 1]                                           # strided: four doubles, 24 bytes apart
    assert not column.is_contiguous()
    cases.insert(4, column)
    return cases


def check(got, tensors):
    """Every piece holds its tensor's exact bytes in its tensor's dtype and shape, aligned and writable."""
    assert isinstance(got, list) and len(got) == len(tensors)
    for piece, t in zip(got, tensors):
        want = t.cpu().contiguous().numpy()
        assert isinstance(piece, np.ndarray) and piece.dtype == want.dtype and piece.shape == want.shape
        assert piece.tobytes() == want.tobytes()
        assert piece.flags.aligned and piece.flags.c_contiguous and piece.flags.writeable
