"""The per-env setter pattern, once: pick envs by `env_mask` or `env_ids`, turn an int, array or tensor into one value per picked
env, check what lives on the host and only guard what lives on the device, write the rows.  Plain functions over numpy arrays
(`device=None`: the `_dry` form) or torch tensors of `device`; `who` / `label` are the caller's names in the messages.  Used by
set_params, set_levels, reset(env_mask=), set_agent, LevelBank.assign and the sharded splits (sharding.split_params)."""
import numpy as np


def host_ints(v, what, wide=True):
    """host values -> integer ndarray; ValueError for anything that is no integer (bools included).  `wide`: python ints up to
    2**63 - 1 in object arrays and uint64 are taken too, and the result is int64."""
    a = np.asarray(v.cpu() if hasattr(v, "cpu") else v)
    if wide and a.dtype == object:
        try:
            a = a.astype(np.int64)
        except (OverflowError, TypeError, ValueError):
            raise ValueError("%s: integers in [-1, 2**63 - 1]" % what)
    if a.dtype.kind not in "iu" or a.dtype == bool:
        raise ValueError("%s: integer values, not %s" % (what, a.dtype))
    if not wide:
        return a
    if a.dtype == np.uint64 and a.size and a.max() > np.uint64(2 ** 63 - 1):
        raise ValueError("%s: integers in [-1, 2**63 - 1]" % what)
    return a.astype(np.int64)


def on_device(v, device):
    """a tensor that already lives on a GPU: nothing of it is read on the host"""
    return device is not None and hasattr(v, "is_cuda") and v.is_cuda


def to_device(a, device):
    """a host array as it is (`device` None), or as a tensor of `device`"""
    if device is None:
        return a
    import torch
    return torch.from_numpy(a if a.ndim == 0 else np.ascontiguousarray(a)).to(device)       # (ascontiguousarray: ndim >= 1)


def shape_of(v):
    return tuple(v.shape) if hasattr(v, "shape") else np.shape(v)


def check_selectors(B, env_mask, env_ids, who):
    if env_mask is not None and env_ids is not None:
        raise ValueError("%s: env_mask or env_ids, not both" % who)
    if env_mask is not None and shape_of(env_mask) != (B,):
        raise ValueError("env_mask must have shape (batch_size,)")


def host_ids(env_ids, B, who, any_number=False):
    """`env_ids` on the host: (k,) int64, every one in 0 .. B-1.  `any_number`: whatever numpy casts to int64 is taken (an
    empty list, floats), as set_params and the splits always did; otherwise integers only (`host_ints`)."""
    if any_number:
        ids = np.asarray(env_ids.cpu() if hasattr(env_ids, "cpu") else env_ids).astype(np.int64).reshape(-1)
    else:
        ids = host_ints(env_ids, "%s(env_ids=)" % who).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= B):
        raise ValueError("%s: env_ids outside 0..%d" % (who, B - 1))
    return ids


def select(B, device, env_mask, env_ids, who, any_number=False):
    """(mask, ids) of a per-env setter, at most one of them: `mask` (B,) bytes 0 / 1 — an integer mask selects where it is
    nonzero —, `ids` (k,) int64.  Host ids are range-checked; a device tensor is only moved and flattened, nothing is read back,
    and a bool device tensor (step()'s `done`) is taken as it is, without a launch."""
    check_selectors(B, env_mask, env_ids, who)
    mask = ids = None
    if on_device(env_mask, device):
        import torch
        mask = env_mask.to(device)
        mask = (mask if mask.dtype == torch.bool else mask != 0).contiguous().view(torch.uint8)
    elif env_mask is not None:
        mask = to_device(np.asarray(env_mask.cpu() if hasattr(env_mask, "cpu") else env_mask).astype(bool).view(np.uint8), device)
    if on_device(env_ids, device):
        ids = env_ids.to(device).long().reshape(-1)
    elif env_ids is not None:
        ids = to_device(host_ids(env_ids, B, who, any_number), device)
    return mask, ids


def check_value_shape(shape, B, k, label):
    """an int, one value per selected env, or — with `env_ids` — one per env of the batch"""
    want = (B,) if k is None else (k,)
    if shape not in ((), want, (B,)):
        raise ValueError("%s: an int or one value per env, shape %s; got %s" % (label, want, shape))


def values(v, lo, hi, B, ids, device, label, interval, dtype=np.int64, wide=True, clamp=False):
    """`v` as a 0-d or (k,) array / tensor of `dtype`, k the number of selected envs (B without `ids`; a (B,) value given with
    `ids` is gathered by them).  Host values are checked against [lo, hi) — `hi` None: no upper end — and refused with
    "<label>: values a..b outside <interval>"; a device tensor is clamped to it (`clamp`) or passed through, for the device to
    guard."""
    if on_device(v, device):
        import torch
        v = v.to(device)
        v = (v.clamp(lo, hi - 1) if clamp else v).to(getattr(torch, np.dtype(dtype).name))
    else:
        v = host_ints(v, label, wide)
        if v.size and (v.min() < lo or (hi is not None and v.max() >= hi)):
            raise ValueError("%s: values %d..%d outside %s" % (label, v.min(), v.max(), interval))
        v = to_device(v.astype(dtype), device)
    k = None if ids is None else int(ids.shape[0])
    if k is not None and tuple(v.shape) == (B,) != (k,):
        v = v[ids]
    check_value_shape(tuple(v.shape), B, k, label)
    return v


def write(dst, v, mask, ids):
    """`dst[ids] = v`, `dst` where `mask`, or all of `dst` — in place, one op each"""
    if ids is not None:
        dst[ids] = v
    elif isinstance(dst, np.ndarray):
        dst[...] = v if mask is None else np.where(mask.view(bool), v, dst)
    elif mask is None:
        dst.copy_(v)
    else:
        import torch
        torch.where(mask.view(torch.bool), v, dst, out=dst)
