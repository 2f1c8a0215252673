"""How the stage wrappers judge their arguments, in one place: which GPU a call runs on, "is this a dtype-X tensor of this shape
on the device of the others", an ascending class list.  The order of judgement is fixed -- type, dtype, shape, contiguity and
only then the device -- so whatever can be judged without a GPU is a ValueError with or without one, and a well-formed host
tensor is the AcrHipError of ``_lib.require_gpu`` (there is no CPU path).  A stage's own rules stay in its module.  torch is
imported where it is used: ``evaluation`` imports this module and stays importable for its numpy half."""
import ctypes

import numpy as np

from . import _abi

MAX_SEG_CLASSES = _abi.constants["ACR_SEG_MAX_K"]   # 2 <= K <= 128: the logits segloss trains on and segval predicts from


def gpu_device(device, what):
    """``device`` as a torch.device("cuda", index), else AcrHipError: ``what`` has no CPU path."""
    import torch
    from ._lib import AcrHipError
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise AcrHipError("%s needs a GPU (got device %r): there is no CPU path" % (what, device))
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def first_device(tensors, device, what):
    """The GPU a call runs on: that of the first tensor among ``tensors`` (AcrHipError if it is a host tensor), else ``device``."""
    import torch
    from ._lib import require_gpu
    for t in tensors:
        if torch.is_tensor(t):
            require_gpu(t)
            return t.device
    return gpu_device(device, what)


def on_device(x, name, device=None, upload=False):
    """The last two steps of ``tensor_arg`` for a tensor judged earlier: on a GPU (a host tensor goes to ``device`` first when
    ``upload`` is set), and on ``device`` if one is given."""
    from ._lib import require_gpu
    if upload and device is not None and not x.is_cuda:
        x = x.to(device, non_blocking=True)
    require_gpu(x)
    if device is not None and x.device != device:
        raise ValueError("%s lies on %s, the other inputs on %s" % (name, x.device, device))
    return x


def tensor_arg(x, name, dtype, *, shape=None, contiguous=True, device=None, upload=False, bool_as_u8=False, on_gpu=True):
    """``x`` as the tensor to hand to the library: a non-empty ``dtype`` tensor (``bool_as_u8``: bool counts as uint8) of ``shape``
    -- an integer entry must match, a string names a free axis: (3, "W", "H") --, contiguous unless told otherwise, on a GPU, and
    on ``device`` if one is given.  ``upload``: a numpy array is taken too and copied to ``device``.  ``on_gpu=False`` stops before
    the device is looked at, for a caller that has more arguments to judge first (it finishes with ``on_device``)."""
    import torch
    kind = ("contiguous " if contiguous else "") + str(dtype)[len("torch."):]
    host = not torch.is_tensor(x)
    if host:
        if not upload:
            raise ValueError("%s must be a torch tensor on the GPU, got %s" % (name, type(x).__name__))
        x = np.asarray(x)
        if x.dtype != getattr(np, kind.split()[-1]) and not (bool_as_u8 and x.dtype == np.bool_):
            raise ValueError("%s must be %s, got %s" % (name, kind, x.dtype))
        x = torch.from_numpy(np.ascontiguousarray(x))
    if bool_as_u8 and x.dtype == torch.bool:
        x = x.contiguous().view(torch.uint8)
    if x.dtype != dtype:
        raise ValueError("%s must be a %s tensor, got %s with strides %s" % (name, kind, x.dtype, tuple(x.stride())))
    fits = shape is None or (x.dim() == len(shape) and all(isinstance(s, str) or s == n for s, n in zip(shape, x.shape)))
    if not fits or x.numel() == 0:
        want = "" if shape is None else "(%s) " % ", ".join(str(s) for s in shape)
        raise ValueError("%s must be a non-empty %stensor, got %s" % (name, want, tuple(x.shape)))
    if contiguous and not x.is_contiguous():
        raise ValueError("%s must be a %s tensor, got %s with strides %s" % (name, kind, x.dtype, tuple(x.stride())))
    return on_device(x, name, device, upload=host) if on_gpu else x


def class_array(classes, n_classes, what):
    """(ctypes int32 array, list) of a strictly ascending list of class ids below ``n_classes``; ``what``: what an image without a
    class lacks."""
    cl = [int(c) for c in classes]
    if not cl:
        raise ValueError("no classes: an image without a positive class has %s" % what)
    if any(c < 0 or c >= n_classes for c in cl):
        raise ValueError("classes %s outside 0..%d" % (cl, n_classes - 1))
    if any(b <= a for a, b in zip(cl, cl[1:])):
        raise ValueError("classes %s must be strictly ascending (sorted, no duplicates)" % (cl,))
    return (ctypes.c_int32 * len(cl))(*cl), cl
