"""Array arguments of the C ABI (include/copra_hip.h), for batch.py: host array or device tensor, and what a shape means.

A numpy array (anything numpy converts) is COPIED: contiguous, of the ABI's dtype, matrices transposed from natural indexing to the ABI's
column-major -- the library gets on_device = 0 and copies again, so the copy lives for the call.  A torch tensor is used IN PLACE: it must be
resident on the device, contiguous, of the dtype and in ABI layout already; the library gets on_device = 1 and reads the memory later, so the
caller of marshal() keeps Arg.owner alive (BatchLMPC._hold).  Pure: numpy only, nothing here loads the library or torch."""
import collections

import numpy as np

from ._capi import CopraDomainError

# ptr: what the library gets; on_device: 0 a host copy, 1 the caller's tensor; shape: in natural indexing; owner: the object that owns the memory
Arg = collections.namedtuple("Arg", "ptr on_device shape owner")


def is_torch(t):
    return type(t).__module__.startswith("torch")


def is_resident(t):
    """whether the library's kernels can read tensor `t` in place (the one residency test: CPU tests replace it)"""
    return t.is_cuda


def marshal(a, what, dtype="float64", matrix=False):
    """the Arg of array or tensor `a` (None: None).  matrix: the last two axes are a matrix in natural indexing -- a numpy array is transposed
    to column-major, a tensor holds column-major already and its shape is reported back in natural indexing."""
    if a is None:
        return None
    tensor = is_torch(a)
    if tensor:
        if not (is_resident(a) and a.is_contiguous() and str(a.dtype) == "torch." + dtype):
            raise ValueError("%s: a contiguous CUDA %s tensor is needed" % (what, dtype))
        owner, ptr = a, a.data_ptr()
    else:
        owner = np.asarray(a, dtype=dtype)
        owner = np.ascontiguousarray(np.swapaxes(owner, -1, -2) if matrix and owner.ndim >= 2 else owner)
        ptr = owner.ctypes.data
    shape = tuple(owner.shape)
    if matrix and len(shape) >= 2:
        shape = shape[:-2] + (shape[-1], shape[-2])
    return Arg(ptr, int(tensor), shape, owner)


def expect(arg, shape, what):
    """`arg`, which must have `shape`"""
    if arg.shape != tuple(shape):
        raise CopraDomainError("%s: expected %s, got %s" % (what, tuple(shape), arg.shape))
    return arg


def weight_form(shape, r, batch, what="weight", dense_allowed=True):
    """(dense, per_instance) of a weight over r rows: (r,) diagonal, (r, r) dense, (batch, r) / (batch, r, r) one per instance; with
    batch == r a 2-d array is read as (r, r).  dense_allowed=False: a vector of r rows, (r,) or (batch, r)."""
    forms = [((r,), 0, 0), ((r, r), 1, 0), ((batch, r), 0, 1), ((batch, r, r), 1, 1)]
    for form, dense, per in forms:
        if tuple(shape) == form and (dense_allowed or not dense):
            return dense, per
    raise CopraDomainError("%s: expected %s, got %s" % (what, " or ".join(str(f) for f, d, _ in forms if dense_allowed or not d), tuple(shape)))


def signal_form(shape, r, batch, constant_allowed, what="signal"):
    """(steps, per_instance) of a signal of r rows: (steps, r) one for the batch, (batch, steps, r) one per instance, and where a constant is
    allowed (r,): one step"""
    shape = tuple(shape)
    if constant_allowed and shape == (r,):
        return 1, 0
    if len(shape) == 2 and shape[1] == r and shape[0] >= 1:
        return shape[0], 0
    if len(shape) == 3 and shape[0] == batch and shape[2] == r and shape[1] >= 1:
        return shape[1], 1
    raise CopraDomainError("%s: expected %s(steps, %d) or (%d, steps, %d), got %s" % (what, "(%d,), " % r if constant_allowed else "", r, batch, r, shape))


def weight(a, r, batch, what, dense_allowed=True):
    """(Arg, dense, per_instance) of weight `a`: its form decides whether it is a matrix"""
    arg = marshal(a, what)
    dense, per = weight_form(arg.shape, r, batch, what, dense_allowed)
    if dense and not arg.on_device:
        arg = marshal(arg.owner, what, matrix=True)
    return arg, dense, per


def signal(a, r, batch, constant_allowed, what):
    """(Arg, steps, per_instance) of signal `a`"""
    arg = marshal(a, what)
    return (arg,) + signal_form(arg.shape, r, batch, constant_allowed, what)


def same_way(what, args, pers=(), mixed_per=CopraDomainError):
    """(on_device, per_instance) of arrays that share one flag of each: `args` all host copies or all tensors (ValueError), their
    per-instance flags `pers` all equal (mixed_per)"""
    args = [a for a in args if a is not None]
    if len({a.on_device for a in args}) > 1:
        raise ValueError("%s: the arrays are all numpy or all torch CUDA tensors" % what)
    if len(set(pers)) > 1:
        raise mixed_per("%s: the arrays are all given once or all per instance (tensors are used in place)" % what)
    return args[0].on_device, int(next(iter(pers), 0))


# ---- numpy only: what a host copy can become before the call (a tensor is used as it is) ----
def written_out(arg, batch):
    """a host array given once, written out per instance"""
    a = np.ascontiguousarray(np.broadcast_to(arg.owner, (batch,) + arg.owner.shape))
    return Arg(a.ctypes.data, 0, (batch,) + arg.shape, a)


def diagonal_as_dense(arg):
    """a host diagonal weight (.., r) as the dense (.., r, r)"""
    a = np.ascontiguousarray(arg.owner[..., None] * np.eye(arg.shape[-1]))
    return Arg(a.ctypes.data, 0, arg.shape + arg.shape[-1:], a)
