"""Where the data layer's arrays live: the one device rule, the host / device forms of a log column and of a store's named
arrays, and the build= switch.  dataprep, targets, graph, pointdata and logremap all take these from here; the module imports
nothing else of the package, and torch only inside the functions that need a device.
"""
import numpy as np


def is_tensor(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "data_ptr")


def to_host(a):
    return a.cpu().numpy() if is_tensor(a) else np.asarray(a)


def check_build(build, message=None):
    """ValueError unless build is "host" or "device"; message: a caller's own text for it"""
    if build not in ("host", "device"):
        raise ValueError(message if message is not None else "build is 'host' or 'device': got %r" % (build,))


NO_CPU_PATH = "batch assembly has no CPU path"


def device_of(device=None, what="build='device'", like=None, instead="build='host' does not"):
    """the torch device of a device build: `device` where given, else the device of `like` where that is a tensor on one, else
    the current device.  RuntimeError without a GPU: "<what> needs an AMD GPU (HIP); <instead>"."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("%s needs an AMD GPU (HIP); %s" % (what, instead))
    if device is None and is_tensor(like) and like.is_cuda:
        device = like.device
    return torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())


def device_i32(a, dev):
    """a column of the log as a flat int32 tensor on `dev`: a tensor is used where it is (converted or moved only if it has
    to be), anything else goes through numpy and is uploaded"""
    import torch
    if is_tensor(a):
        return a.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).ravel(), dtype=np.int32)).to(dev)


def device_as(a, dev, dtype=None):
    """an array in its own shape as a tensor on `dev`: a tensor is the object's own where it lives there (moved otherwise),
    numpy is uploaded, as `dtype` where one is given"""
    import torch
    return a.to(dev) if is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def upload_named(names, get, dev):
    """a store's named arrays as tensors on `dev` -> {name: tensor}: get(name) is numpy (uploaded), a tensor (.to(dev): the
    very tensor where it lives there) or None (left out -- its pointer in the argument struct is null); an EMPTY array is a
    one-word int32 zero tensor, so that the struct still holds a valid pointer for it"""
    import torch
    d = {}
    for k in names:
        a = get(k)
        if a is None:
            continue
        if (a.numel() if is_tensor(a) else np.size(a)) == 0:
            d[k] = torch.zeros((1,), dtype=torch.int32, device=dev)
        else:
            d[k] = device_as(a, dev)
    return d
