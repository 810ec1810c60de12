"""Padded batches of 1-D clips of unequal length: what every list function does around its one Engine call -- convert, order by
length, cut into batches, pad, and hand each row back.  Plain functions on NumPy arrays and torch tensors; no Engine, no GPU."""
import numpy as np
import torch


def as_tensor(c):
    """A clip (NumPy array or tensor) as a tensor, where it is."""
    return c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c))


def as_numpy(c):
    """A clip (NumPy array or tensor, on any device) as a NumPy array on the host."""
    return c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)


def is_f32(c):
    return str(c.dtype).endswith("float32")


def to_device(y, device):
    """A host result (or a tensor) as a tensor on `device`."""
    return as_tensor(y).to(device)


def batches(indices, lengths, max_batch):
    """`indices` ascending by lengths[i] -- stable: equal lengths keep the caller's order -- in lists of at most `max_batch`."""
    order = sorted(indices, key=lambda i: lengths[i])
    for k in range(0, len(order), max_batch):
        yield order[k:k + max_batch]


def pad(rows, device, dtype, width=None):
    """1-D rows -> a zero-filled (len(rows), width) tensor on `device` with row j in [:len_j]; width defaults to the longest row."""
    if width is None:
        width = max(r.shape[0] for r in rows)
    x = torch.zeros((len(rows), width), device=device, dtype=dtype)
    for j, r in enumerate(rows):
        x[j, :r.shape[0]] = as_tensor(r).to(device=device, dtype=dtype)
    return x


def unpad(y, lengths, to_host):
    """The rows y[j, :lengths[j]] of a batch: copies on the host after ONE download (to_host), or views of the device tensor."""
    if to_host:
        y = y.cpu().numpy()
        return [y[j, :n].copy() for j, n in enumerate(lengths)]
    return [y[j, :n] for j, n in enumerate(lengths)]
