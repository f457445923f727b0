"""The search's "host" | "device" switches, named once.  ``MicArray.__init__`` describes what each one moves to the
GPU; ``MicArray``, ``JointModel`` and ``joint.config_key`` loop over ``MODE_NAMES`` and validate through
``check_modes``, so a further mode is one more name here, its paragraph there and the stage that branches on it."""

# the order is the order ``joint.config_key`` appends the non-default ones in
MODE_NAMES = ("geometry", "segments", "clustering", "global_clustering", "coarse")
# the Prone_methods whose stage 1 is the whole coarse TDoA lattice ("DENSE_NMS": its coarse stage keeps the local maxima)
LATTICE_METHODS = ("DENSE", "DENSE_NMS")


def check_modes(geometry="host", segments="host", clustering="host", global_clustering="host", coarse="host",
                Prone_method=None):
    """The five values, after refusing (``ValueError``) a value that is neither "host" nor "device" and a combination
    that cannot run.  ``Prone_method``: the pruning method the modes will search with, where it is known already."""
    values = (geometry, segments, clustering, global_clustering, coarse)
    for name, value in zip(MODE_NAMES, values):
        if value not in ("host", "device"):
            raise ValueError(f'{name} must be "host" or "device", got {value!r}')
    if global_clustering == "device" and segments != "device":
        raise ValueError('global_clustering="device" needs segments="device"')
    if coarse == "device" and Prone_method is not None and Prone_method not in LATTICE_METHODS:
        raise ValueError(f'coarse="device" needs a lattice search (Prone_method in {LATTICE_METHODS}), got {Prone_method!r}')
    return values


def need_methods(obj, keyword, *methods):
    """``RuntimeError`` unless ``obj`` has every one of ``methods``: a duck-typed spot model cannot serve the mode
    ``keyword`` (written as at the call, e.g. ``'clustering="device"'``), and there is no quiet fall-back to the host path."""
    if not all(hasattr(obj, m) for m in methods):
        raise RuntimeError(f'{keyword} needs a spot model with {" and ".join(m + "()" for m in methods)} (the HIP SpotModel)')
