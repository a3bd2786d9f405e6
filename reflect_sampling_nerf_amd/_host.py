"""Host-side helpers the export tools and the checkpoint writer share."""
import contextlib
import os

import numpy as np
import torch


def _np(x, dtype):
    """Tensor or array -> contiguous numpy array of `dtype` on the host."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


@contextlib.contextmanager
def replacing(path: str):
    """-> the temporary name path + ".tmp" to write to; it is renamed to `path` when the block ends without an error, so a reader
    never sees a half-written file."""
    yield path + ".tmp"
    os.replace(path + ".tmp", path)
