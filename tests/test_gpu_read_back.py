"""GPU: ``native.read_back`` brings device tensors of mixed dtypes over in one copy, byte for byte."""
import pytest
import torch

from tests.read_back_cases import check, make_cases

pytestmark = pytest.mark.gpu


def test_read_back_on_device_tensors():
    from acousticswarms_speech_amd.native import read_back
    cases = make_cases("cuda")
    assert all(t.is_cuda for t in cases)
    check(read_back(*cases), cases)                   # against each tensor's own .cpu().numpy()
    check(read_back(*cases[::-1]), cases[::-1])
    for t in cases:
        check(read_back(t), [t])
    assert read_back() == []
    # the shapes of the two stages that use it: (kept, counts, thr, best, degree) and (energies, order, label)
    g = torch.Generator().manual_seed(3)
    coarse = [torch.randint(-1, 99, (30,), generator=g, dtype=torch.int32), torch.tensor([31, 0], dtype=torch.int32),
              torch.tensor([0.008, float("nan")], dtype=torch.float64),
              torch.randint(0, 3364, (3364,), generator=g, dtype=torch.int32),
              torch.randint(0, 729, (3364,), generator=g, dtype=torch.int32)]
    fine = [torch.rand((257, 2), generator=g, dtype=torch.float64), torch.randperm(257, generator=g).to(torch.int32),
            torch.randint(-1, 257, (257,), generator=g, dtype=torch.int32)]
    for group in (coarse, fine):
        dev = [t.cuda() for t in group]
        check(read_back(*dev), group)
