"""Oracle mask fixture (g16): run the REFERENCE's own ``do_irm`` (sep/helpers/irm.py) and ``do_ibm`` (sep/helpers/ibm.py)
on seeded inputs and record what they return.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_masks.py

Two adaptations, both made in this process before the import and neither touching the reference's text: the two files
say ``np.float``, which numpy 2 removed, so ``np.float = float`` is set; and they import ``tqdm`` without using it, so
an empty module of that name is put into ``sys.modules`` when the package is absent.

The inputs are float32 -- two Gaussian sources of N = 4096 samples and their sum plus 10 % noise -- and the two outputs
float64 [2, N], with alpha = 1 for both and theta = 0.5 for the binary mask.  The generator refuses inputs with a bin
whose binary-mask ratio lies within 1e-9 (relative) of theta: there the decision could fall either way under a
different FFT.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SEED, N, S = 16, 4096, 2
ALPHA, THETA = 1.0, 0.5


def inputs():
    rng = np.random.default_rng(SEED)
    gt = rng.standard_normal((S, N)).astype(np.float32)
    mix = (gt.astype(np.float64).sum(axis=0) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    return gt, mix


def main():
    sys.path.insert(0, ROOT)
    from tests.golden import make_golden  # noqa: F401    puts the reference on sys.path
    if not hasattr(np, "float"):
        np.float = float                                   # adaptation 1 (module docstring)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.ModuleType("tqdm")     # adaptation 2
    from sep.helpers.ibm import do_ibm
    from sep.helpers.irm import do_irm
    from acousticswarms_speech_amd.oracle_masks import ibm_ratio_f64

    gt, mix = inputs()
    margin = float(np.min(np.abs(ibm_ratio_f64(gt, mix, ALPHA) / THETA - 1.0)))
    assert margin > 1e-9, f"a bin sits {margin:.1e} from the threshold: choose another seed"
    g, m = gt.astype(np.float64)[:, None, :], mix.astype(np.float64)[None, :]            # (n_voices, 1, t) and (1, t)
    irm = np.asarray(do_irm(g, m, alpha=ALPHA), dtype=np.float64).reshape(S, N)
    ibm = np.asarray(do_ibm(g, m, ALPHA, THETA), dtype=np.float64).reshape(S, N)
    path = os.path.join(HERE, "g16_oracle_masks.npz")
    np.savez_compressed(path, gt=gt, mix=mix, irm=irm, ibm=ibm, alpha=np.float64(ALPHA), theta=np.float64(THETA),
                        seed=np.int64(SEED), margin=np.float64(margin))
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB); nearest bin {margin:.2e} from theta")


if __name__ == "__main__":
    main()
