"""`dsc.Tensor` and its operators (mirror of python/dsc/tensor.py: Tensor :159-331, from_numpy :371-377,
reshape / concat :380-404, add .. power :459-501, cos .. sqrt :504-533, i0 / clip :560-576, sum/mean/max/min :579-612,
arange / randn :615-620, fft/ifft/rfft/irfft :693-726).

Differences forced by the device arena (see include/dsc_mi355x.h): `numpy()` and
`from_numpy()` COPY through dsc_copy_to_host / dsc_copy_from_host instead of viewing /
memmoving the data pointer."""
import builtins
from typing import List, Tuple, Union

import numpy as np

from . import _bindings as B
from .context import _current as _current_ctx
from .context import _get_ctx
from .dtype import DTYPE_CONVERSION_TABLES, DTYPE_TO_NP, NP_TO_DTYPE, Dtype, ScalarType

TensorType = Union['Tensor', np.ndarray]
_DSC_MAX_DIMS = 4


def _c_ptr_or_none(x):
    return x._c_ptr if x is not None else None


class Tensor:
    def __init__(self, c_ptr, view: bool = False):
        # `view=True`: the operator returned the caller's `out`; make a second handle on the
        # same buffer so that both can be freed (python/dsc/tensor.py:160-161).
        c_ptr = c_ptr if not view else B.dsc_view(_get_ctx(), c_ptr)
        c = c_ptr.contents
        self._dtype = Dtype(c.dtype)
        self._n_dim = c.n_dim
        self._shape = tuple(c.shape[_DSC_MAX_DIMS - c.n_dim:])
        self._ne = c.ne
        self._c_ptr = c_ptr
        # the context (and its clear() epoch) this handle belongs to: it is freed against THAT context only
        self._owner = _current_ctx()
        self._epoch = self._owner.epoch if self._owner is not None else -1

    def __del__(self):
        # Never create a context from a destructor, never free into a context that has been cleared or replaced since
        # this handle was made (dsc_ctx_clear already released it; its header address may belong to a new tensor).
        try:
            owner = self._owner
            if owner is not None and owner is _current_ctx() and owner._ctx and owner.epoch == self._epoch:
                B.dsc_tensor_free(owner._ctx, self._c_ptr)
        except Exception:      # interpreter teardown
            pass

    @property
    def dtype(self) -> Dtype:
        return self._dtype

    @property
    def shape(self) -> Tuple[int, ...]:
        return self._shape

    @property
    def n_dim(self) -> int:
        return self._n_dim

    @property
    def ne(self) -> int:
        return self._ne

    def __len__(self) -> int:
        return self._shape[0]

    def __str__(self) -> str:
        return str(self.numpy())

    def __mul__(self, other):
        return mul(self, other)

    def __rmul__(self, other):
        return mul(other, self)

    def __add__(self, other):
        return add(self, other)

    def __radd__(self, other):
        return add(other, self)

    def __sub__(self, other):
        return sub(self, other)

    def __rsub__(self, other):
        return sub(other, self)

    def __truediv__(self, other):
        return true_div(self, other)

    def __rtruediv__(self, other):
        return true_div(other, self)

    def __pow__(self, other):                                     # python/dsc/tensor.py:293-297
        return power(self, other)

    def __rpow__(self, other):
        return power(other, self)

    def __getitem__(self, item):
        """python/dsc/tensor.py:193-229: ints -> dsc_tensor_get_idx (a fully indexed element is unwrapped to a
        Python scalar), slices or mixed -> dsc_tensor_get_slice.  The copy happens on the device."""
        ctx = _get_ctx()
        if isinstance(item, int):
            return _unwrap(Tensor(B.dsc_tensor_get_idx(ctx, self._c_ptr, item)))
        if isinstance(item, tuple) and all(isinstance(i, int) for i in item):
            return _unwrap(Tensor(B.dsc_tensor_get_idx(ctx, self._c_ptr, *item)))
        if isinstance(item, slice):
            return Tensor(B.dsc_tensor_get_slice(ctx, self._c_ptr, _c_slice(item)))
        if isinstance(item, tuple) and all(isinstance(i, (int, slice)) for i in item):
            return Tensor(B.dsc_tensor_get_slice(ctx, self._c_ptr, *[_c_slice(i) for i in item]))
        raise RuntimeError(f'cannot index Tensor with object {item}')

    def __setitem__(self, key, value):
        """python/dsc/tensor.py:231-270"""
        ctx = _get_ctx()
        val = _wrap(value, self._dtype)
        if val.dtype != self._dtype:
            val = val.cast(self._dtype)
        if isinstance(key, int):
            B.dsc_tensor_set_idx(ctx, self._c_ptr, val._c_ptr, key)
        elif isinstance(key, tuple) and all(isinstance(i, int) for i in key):
            B.dsc_tensor_set_idx(ctx, self._c_ptr, val._c_ptr, *key)
        elif isinstance(key, slice):
            B.dsc_tensor_set_slice(ctx, self._c_ptr, val._c_ptr, _c_slice(key))
        elif isinstance(key, tuple) and all(isinstance(i, (int, slice)) for i in key):
            B.dsc_tensor_set_slice(ctx, self._c_ptr, val._c_ptr, *[_c_slice(i) for i in key])
        else:
            raise RuntimeError(f'cannot index Tensor with object {key}')

    def numpy(self) -> np.ndarray:
        """Device -> host copy (the reference returns a zero-copy view, tensor.py:305-323)."""
        out = np.empty(self._shape if self._n_dim > 0 else (1,), dtype=DTYPE_TO_NP[self._dtype])
        B.dsc_copy_to_host(_get_ctx(), self._c_ptr, out.ctypes.data, out.nbytes)
        return out

    def tobytes(self) -> bytes:
        return self.numpy().tobytes()

    def __bytes__(self) -> bytes:
        return self.tobytes()

    def cast(self, dtype: Dtype) -> 'Tensor':
        out_ptr = B.dsc_cast(_get_ctx(), self._c_ptr, dtype.value)
        same = B.ctypes.cast(out_ptr, B.c_void_p).value == B.ctypes.cast(self._c_ptr, B.c_void_p).value
        return Tensor(out_ptr, view=same)

    def reshape(self, *shape) -> 'Tensor':                        # python/dsc/tensor.py:328-329
        return reshape(self, *shape)


def _unwrap(x: Tensor):
    """python/dsc/tensor.py:91-103: a 1-element 1-D tensor becomes a Python scalar (one device -> host copy)."""
    if x.n_dim != 1 or len(x) != 1:
        return x
    v = x.numpy()[0]
    return complex(v) if np.iscomplexobj(v) else float(v)


def _c_slice(x) -> 'B._DscSlice':
    """python/dsc/tensor.py:106-118: None -> DSC_VALUE_NONE; an int inside a mixed key -> (i, i, i)."""
    if isinstance(x, slice):
        f = lambda i: B.DSC_VALUE_NONE if i is None else int(i)      # noqa: E731
        return B._DscSlice(f(x.start), f(x.stop), f(x.step))
    return B._DscSlice(int(x), int(x), int(x))


def _create_tensor(dtype: Dtype, *dims: int) -> Tensor:
    if not 1 <= len(dims) <= _DSC_MAX_DIMS:
        raise RuntimeError(f'cannot create a Tensor with {len(dims)} dimensions, max is {_DSC_MAX_DIMS}')
    f = (B.dsc_tensor_1d, B.dsc_tensor_2d, B.dsc_tensor_3d, B.dsc_tensor_4d)[len(dims) - 1]
    return Tensor(f(_get_ctx(), dtype.value, *dims))


def empty(shape, dtype: Dtype = Dtype.F32) -> Tensor:
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return _create_tensor(dtype, *shape)


def from_numpy(x: np.ndarray) -> Tensor:
    if x.dtype not in NP_TO_DTYPE:
        raise RuntimeError(f'NumPy dtype {x.dtype} is not supported')
    x = np.ascontiguousarray(x)
    out = _create_tensor(NP_TO_DTYPE[x.dtype], *(x.shape if x.ndim > 0 else (1,)))
    B.dsc_copy_from_host(_get_ctx(), out._c_ptr, x.ctypes.data, x.nbytes)
    return out


def _wrap(x, dtype: Union[Dtype, None] = None) -> Tensor:
    if isinstance(x, np.ndarray):
        return from_numpy(x)
    if isinstance(x, Tensor):
        return x
    ctx = _get_ctx()
    if isinstance(x, complex):
        if dtype == Dtype.C64:
            return Tensor(B.dsc_wrap_c64(ctx, B._C64(x.real, x.imag)))
        return Tensor(B.dsc_wrap_c32(ctx, B._C32(x.real, x.imag)))
    if dtype == Dtype.F64:
        return Tensor(B.dsc_wrap_f64(ctx, float(x)))
    if dtype == Dtype.C32:
        return Tensor(B.dsc_wrap_c32(ctx, B._C32(float(x), 0.0)))
    if dtype == Dtype.C64:
        return Tensor(B.dsc_wrap_c64(ctx, B._C64(float(x), 0.0)))
    return Tensor(B.dsc_wrap_f32(ctx, float(x)))


def _wrap_operands(xa, xb) -> Tuple[Tensor, Tensor]:
    # python/dsc/tensor.py:435-458
    def _dtype(x) -> Dtype:
        if isinstance(x, Tensor):
            return x.dtype
        if isinstance(x, np.ndarray):
            return NP_TO_DTYPE[x.dtype]
        if isinstance(x, (int, float)):
            return Dtype.F32
        return Dtype.C32

    if (isinstance(xa, Tensor) and isinstance(xb, Tensor)) or (isinstance(xa, np.ndarray) and isinstance(xb, np.ndarray)):
        return _wrap(xa), _wrap(xb)
    wrap_dtype = DTYPE_CONVERSION_TABLES[_dtype(xa).value][_dtype(xb).value]
    return _wrap(xa, wrap_dtype), _wrap(xb, wrap_dtype)


def _binary(f, xa, xb, out) -> Tensor:
    xa, xb = _wrap_operands(xa, xb)
    return Tensor(f(_get_ctx(), xa._c_ptr, xb._c_ptr, _c_ptr_or_none(out)), out is not None)


def mul(xa, xb, out: Union[Tensor, None] = None) -> Tensor:
    return _binary(B.dsc_mul, xa, xb, out)


def add(xa, xb, out: Union[Tensor, None] = None) -> Tensor:         # python/dsc/tensor.py:461-467
    return _binary(B.dsc_add, xa, xb, out)


def sub(xa, xb, out: Union[Tensor, None] = None) -> Tensor:         # :469-475
    return _binary(B.dsc_sub, xa, xb, out)


def true_div(xa, xb, out: Union[Tensor, None] = None) -> Tensor:    # :485-491
    return _binary(B.dsc_div, xa, xb, out)


def power(xa, xb, out: Union[Tensor, None] = None) -> Tensor:       # :495-501
    return _binary(B.dsc_pow, xa, xb, out)


def _same_ptr(a, b) -> bool:
    return B.ctypes.cast(a, B.c_void_p).value == B.ctypes.cast(b, B.c_void_p).value


def absolute(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:       # python/dsc/tensor.py:530-534
    return Tensor(B.dsc_abs(_get_ctx(), x._c_ptr, _c_ptr_or_none(out)), out is not None)


def angle(x: Tensor) -> Tensor:                                           # :537-538
    return Tensor(B.dsc_angle(_get_ctx(), x._c_ptr))


def conj(x: Tensor) -> Tensor:                                            # :541-544 (a real tensor comes back as a view of itself)
    p = B.dsc_conj(_get_ctx(), x._c_ptr)
    return Tensor(p, view=_same_ptr(p, x._c_ptr))


def real(x: Tensor) -> Tensor:                                            # :547-550
    p = B.dsc_real(_get_ctx(), x._c_ptr)
    return Tensor(p, view=_same_ptr(p, x._c_ptr))


def imag(x: Tensor) -> Tensor:                                            # :553-554
    return Tensor(B.dsc_imag(_get_ctx(), x._c_ptr))


def _unary(f, x: Tensor, out) -> Tensor:
    return Tensor(f(_get_ctx(), x._c_ptr, _c_ptr_or_none(out)), out is not None)


def cos(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:            # python/dsc/tensor.py:504-533
    return _unary(B.dsc_cos, x, out)


def sin(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:
    return _unary(B.dsc_sin, x, out)


def sinc(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:
    return _unary(B.dsc_sinc, x, out)


def logn(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:
    return _unary(B.dsc_logn, x, out)


def log2(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:
    return _unary(B.dsc_log2, x, out)


def log10(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:
    return _unary(B.dsc_log10, x, out)


def exp(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:
    return _unary(B.dsc_exp, x, out)


def sqrt(x: Tensor, out: Union[Tensor, None] = None) -> Tensor:
    return _unary(B.dsc_sqrt, x, out)


def i0(x: Union[int, float, Tensor], dtype: Dtype = Dtype.F32) -> Tensor:       # :560-562: a Python scalar is wrapped first
    x = _wrap(x, dtype)
    return Tensor(B.dsc_i0(_get_ctx(), x._c_ptr))


def clip(x: Tensor, x_min: Union[float, None] = None, x_max: Union[float, None] = None,
         out: Union[Tensor, None] = None) -> Tensor:                                # :565-576: a missing bound is -inf / +inf
    x_min = float(x_min) if x_min is not None else float('-inf')
    x_max = float(x_max) if x_max is not None else float('+inf')
    return Tensor(B.dsc_clip(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), x_min, x_max), out is not None)


def arange(n: int, dtype: Dtype = Dtype.F32) -> Tensor:                  # :615-616
    return Tensor(B.dsc_arange(_get_ctx(), n, dtype.value))


def randn(*shape: int, dtype: Dtype = Dtype.F32) -> Tensor:              # :619-620
    dims = (B.c_int * len(shape))(*shape)
    return Tensor(B.dsc_randn(_get_ctx(), len(shape), dims, dtype.value))


def reshape(x: Tensor, *shape) -> Tensor:                               # :380-391: ints, or one list / tuple of ints
    if len(shape) == 1 and isinstance(shape[0], (tuple, list)) and all(isinstance(s, int) for s in shape[0]):
        dims = tuple(shape[0])
    elif all(isinstance(s, int) for s in shape):
        dims = shape
    else:
        raise RuntimeError(f'cannot reshape tensor with shape {shape}')
    return Tensor(B.dsc_reshape(_get_ctx(), x._c_ptr, *dims))


def concat(tensors, axis: Union[int, None] = 0) -> Tensor:               # :394-404: axis=None flattens
    if isinstance(tensors, (tuple, list)) and all(isinstance(t, Tensor) for t in tensors):
        return Tensor(B.dsc_concat(_get_ctx(), axis if axis is not None else B.DSC_VALUE_NONE, *[t._c_ptr for t in tensors]))
    raise RuntimeError(f'cannot concatenate tensors {tensors}')


def _reduce(f, x: Tensor, out, axis: int, keepdims: bool) -> Tensor:
    return Tensor(f(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), axis, keepdims), out is not None)


def sum(x: Tensor, out=None, axis: int = -1, keepdims: bool = True) -> Tensor:
    return _reduce(B.dsc_sum, x, out, axis, keepdims)


def mean(x: Tensor, out=None, axis: int = -1, keepdims: bool = True) -> Tensor:
    return _reduce(B.dsc_mean, x, out, axis, keepdims)


def max(x: Tensor, out=None, axis: int = -1, keepdims: bool = True) -> Tensor:
    return _reduce(B.dsc_max, x, out, axis, keepdims)


def min(x: Tensor, out=None, axis: int = -1, keepdims: bool = True) -> Tensor:
    return _reduce(B.dsc_min, x, out, axis, keepdims)


def plan_fft(n: int, fft_type: int = 1, dtype: Dtype = Dtype.F64):
    """Build (or touch) the plan for an n-point transform.  fft_type: 0 REAL, 1 COMPLEX.
    (The reference's Python plan_fft passes dtype in the fft_type slot and aborts,
    _bindings.py:88-93 vs dsc.h:139-141; this one follows the C signature.)"""
    return B.dsc_plan_fft(_get_ctx(), n, fft_type, dtype.value)


def _fft_like(f, x: Tensor, out, n: int, axis: int) -> Tensor:
    return Tensor(f(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), n, axis), out is not None)


def fft(x: Tensor, out=None, n: int = -1, axis: int = -1) -> Tensor:
    return _fft_like(B.dsc_fft, x, out, n, axis)


def ifft(x: Tensor, out=None, n: int = -1, axis: int = -1) -> Tensor:
    return _fft_like(B.dsc_ifft, x, out, n, axis)


def rfft(x: Tensor, out=None, n: int = -1, axis: int = -1) -> Tensor:
    return _fft_like(B.dsc_rfft, x, out, n, axis)


def irfft(x: Tensor, out=None, n: int = -1, axis: int = -1) -> Tensor:
    return _fft_like(B.dsc_irfft, x, out, n, axis)


# ---- 2-D transforms over the last two axes (include/dsc_mi355x.h, Section F): numpy.fft.fft2 / ifft2 / rfft2 / irfft2 with
# s = (n0, n1) rounded up to powers of two; None = the axis lengths (irfft2: n1 counts bins, like irfft's n)

def _fft2_like(f, x: Tensor, out, s) -> Tensor:
    n0, n1 = (-1, -1) if s is None else s
    return Tensor(f(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), int(n0), int(n1)), out is not None)


def fft2(x: Tensor, out=None, s=None) -> Tensor:
    return _fft2_like(B.dsc_fft2, x, out, s)


def ifft2(x: Tensor, out=None, s=None) -> Tensor:
    return _fft2_like(B.dsc_ifft2, x, out, s)


def rfft2(x: Tensor, out=None, s=None) -> Tensor:
    return _fft2_like(B.dsc_rfft2, x, out, s)


def irfft2(x: Tensor, out=None, s=None) -> Tensor:
    return _fft2_like(B.dsc_irfft2, x, out, s)


# ---- analytic signal along the last axis (include/dsc_mi355x.h, Section G): scipy.signal.hilbert(x, N) and its absolute value, N = n (None
# or <= 0: the row length) rounded up to a power of two; rows are cropped or zero padded to N

def _hilbert_like(f, x: Tensor, n, out) -> Tensor:
    return Tensor(f(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), -1 if n is None else int(n)), out is not None)


def hilbert(x: Tensor, n: Union[int, None] = -1, out: Union[Tensor, None] = None) -> Tensor:
    """Analytic signal x + i H{x} of every row of real x [.., T]: complex [.., N] whose real part is the (padded / cropped) row."""
    return _hilbert_like(B.dsc_hilbert, x, n, out)


def envelope(x: Tensor, n: Union[int, None] = -1, out: Union[Tensor, None] = None) -> Tensor:
    """|hilbert(x, n)|, real [.., N] of x's dtype, without the complex intermediate."""
    return _hilbert_like(B.dsc_envelope, x, n, out)


# ---- prefix scans along one axis (include/dsc_mi355x.h, Section I): numpy.cumsum / diff / unwrap, and phase = unwrap(angle(z)) fused
def _scan(f, x: Tensor, axis, out) -> Tensor:
    return Tensor(f(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), int(axis)), out is not None)


def cumsum(x: Tensor, axis: int = -1, out: Union[Tensor, None] = None) -> Tensor:
    """numpy.cumsum(x, axis), accumulated in x's dtype (complex component-wise)."""
    return _scan(B.dsc_cumsum, x, axis, out)


def diff(x: Tensor, axis: int = -1, out: Union[Tensor, None] = None) -> Tensor:
    """numpy.diff(x, 1, axis): out[j] = x[j + 1] - x[j]; the axis shrinks by one."""
    return _scan(B.dsc_diff, x, axis, out)


def unwrap(x: Tensor, axis: int = -1, out: Union[Tensor, None] = None) -> Tensor:
    """numpy.unwrap(x, axis=axis) for real x: x - 2 pi K with K the exact integer scan of the whole periods between neighbours."""
    return _scan(B.dsc_unwrap, x, axis, out)


def phase(z: Tensor, axis: int = -1, out: Union[Tensor, None] = None) -> Tensor:
    """unwrap(angle(z), axis) of complex z in one pass: real, bit-identical to the composition."""
    return _scan(B.dsc_phase, z, axis, out)


# ---- moments along one axis (include/dsc_mi355x.h, Section K): every sum in double, var centred on the computed mean (two passes)
def sumsq(x: Tensor, out=None, axis: int = -1, keepdims: bool = True) -> Tensor:
    """sum |x|^2 along the axis in one read; real for complex x."""
    return _reduce(B.dsc_sumsq, x, out, axis, keepdims)


def rms(x: Tensor, out=None, axis: int = -1, keepdims: bool = True) -> Tensor:
    """sqrt(sumsq(x) / n)."""
    return _reduce(B.dsc_rms, x, out, axis, keepdims)


def var(x: Tensor, out=None, axis: int = -1, ddof: int = 0, keepdims: bool = True) -> Tensor:
    """numpy.var(x, axis, ddof=ddof); real for complex x."""
    return Tensor(B.dsc_var(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), int(axis), int(ddof), keepdims), out is not None)


def std(x: Tensor, out=None, axis: int = -1, ddof: int = 0, keepdims: bool = True) -> Tensor:
    """numpy.std(x, axis, ddof=ddof)."""
    return Tensor(B.dsc_std(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), int(axis), int(ddof), keepdims), out is not None)


def vdot(a: Tensor, b: Tensor, out=None, axis: int = -1, keepdims: bool = True) -> Tensor:
    """sum conj(a) b along the axis; a and b of one shape and dtype (no broadcasting)."""
    return Tensor(B.dsc_vdot(_get_ctx(), a._c_ptr, b._c_ptr, _c_ptr_or_none(out), int(axis), keepdims), out is not None)


_DETREND_TYPES = {'constant': 0, 'linear': 1}


def detrend(x: Tensor, axis: int = -1, type: str = 'linear', out: Union[Tensor, None] = None) -> Tensor:
    """scipy.signal.detrend(x, axis, type): the mean ('constant') or the least-squares line ('linear') taken out along the axis."""
    if type not in _DETREND_TYPES:
        raise ValueError(f"type must be 'linear' or 'constant', got {type!r}")
    return Tensor(B.dsc_detrend(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), int(axis), _DETREND_TYPES[type]), out is not None)


# ---- index maps along axes (include/dsc_mi355x.h, Section J): numpy.roll / flip / fft.fftshift / fft.ifftshift / pad in one pass, bit-identical
# to numpy.  Ints or tuples where numpy takes them; `out` must have the result's shape and must not share memory with x.

_PAD_MODES = {'constant': 0, 'edge': 1, 'reflect': 2, 'symmetric': 3, 'wrap': 4}


def _c_ints(values):
    values = [int(v) for v in values]
    return (B.c_int * builtins.max(len(values), 1))(*values)


def _axes_tuple(axis) -> tuple:
    return tuple(int(a) for a in axis) if isinstance(axis, (tuple, list)) else (int(axis),)


def _along_axes(f, x: Tensor, axes, out) -> Tensor:
    if axes is not None and len(_axes_tuple(axes)) == 0:                 # numpy: an empty tuple names no axis, the result is a copy
        return roll(x, 0, axis=0, out=out)
    axes = () if axes is None else _axes_tuple(axes)                    # n_axes == 0: every axis
    return Tensor(f(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), len(axes), _c_ints(axes)), out is not None)


def roll(x: Tensor, shift, axis=None, out: Union[Tensor, None] = None) -> Tensor:
    """numpy.roll(x, shift, axis): shifts of any sign and size; axis=None rolls the flattened tensor and keeps the shape; shift and
    axis broadcast against each other, and a repeated axis adds its shifts."""
    shifts = _axes_tuple(shift)
    if axis is None:
        total = builtins.sum(shifts) % x.ne                              # Python's mod: in [0, ne)
        return Tensor(B.dsc_roll(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), 0, _c_ints([total]), None), out is not None)
    axes = _axes_tuple(axis)
    if len(shifts) != len(axes):
        if len(shifts) != 1 and len(axes) != 1:
            raise ValueError(f'roll: shift {shift} and axis {axis} do not broadcast')
        shifts, axes = shifts * (len(axes) if len(shifts) == 1 else 1), axes * (len(shifts) if len(axes) == 1 else 1)
    if not axes:
        raise ValueError('roll: no axis given')
    # a shift beyond 32 bits is reduced here (the extent of a valid axis); an invalid axis goes through and ends in the library's message
    shifts = [s % x.shape[a] if -x.n_dim <= a < x.n_dim and not -2 ** 31 <= s < 2 ** 31 else s for s, a in zip(shifts, axes)]
    return Tensor(B.dsc_roll(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), len(axes), _c_ints(shifts), _c_ints(axes)), out is not None)


def flip(x: Tensor, axis=None, out: Union[Tensor, None] = None) -> Tensor:
    """numpy.flip(x, axis); axis=None flips every axis."""
    return _along_axes(B.dsc_flip, x, axis, out)


def fftshift(x: Tensor, axes=None, out: Union[Tensor, None] = None) -> Tensor:
    """numpy.fft.fftshift(x, axes): the zero bin to the middle; axes=None shifts every axis."""
    return _along_axes(B.dsc_fftshift, x, axes, out)


def ifftshift(x: Tensor, axes=None, out: Union[Tensor, None] = None) -> Tensor:
    """numpy.fft.ifftshift(x, axes): the inverse of fftshift (they differ on axes of odd length)."""
    return _along_axes(B.dsc_ifftshift, x, axes, out)


def pad(x: Tensor, pad_width, mode: str = 'constant', constant_values=0, out: Union[Tensor, None] = None) -> Tensor:
    """numpy.pad(x, pad_width, mode) for mode 'constant', 'edge', 'reflect', 'symmetric' or 'wrap'; pad_width an int, a (before, after)
    pair or one pair per axis, of any width; constant_values one scalar (complex for complex tensors)."""
    if mode not in _PAD_MODES:
        raise ValueError(f'pad: mode must be one of {sorted(_PAD_MODES)}, got {mode!r}')
    widths = np.asarray(pad_width)
    if widths.dtype.kind not in 'iu':
        raise TypeError('pad: pad_width must be of integral type')
    widths = np.broadcast_to(widths, (x.n_dim, 2))
    value = complex(constant_values)
    return Tensor(B.dsc_pad(_get_ctx(), x._c_ptr, _c_ptr_or_none(out), _c_ints(widths.reshape(-1)), _PAD_MODES[mode], value.real, value.imag),
                  out is not None)


# ---- polyphase FIR resampling along the last axis (include/dsc_mi355x.h, Section H): scipy.signal.upfirdn / resample_poly / decimate
# (ftype='fir') and the low-pass firwin, in one pass of the direct kernel; nothing is rounded to a power of two

_FIRWIN_WINDOWS = {'hamming': 0, 'kaiser': 1}


def upfirdn(h: Tensor, x: Tensor, up: int = 1, down: int = 1, out: Union[Tensor, None] = None) -> Tensor:
    """Upsample every row of real x [.., T] by `up` (zero stuffing), filter with real h [M] of the same dtype, keep every `down`-th
    sample: ceil(((T - 1) up + M) / down) samples per row.  scipy.signal.upfirdn(h, x, up, down, axis=-1)."""
    return Tensor(B.dsc_upfirdn(_get_ctx(), h._c_ptr, x._c_ptr, int(up), int(down), _c_ptr_or_none(out)), out is not None)


def resample_poly(x: Tensor, up: int, down: int, taps: Union[Tensor, None] = None, out: Union[Tensor, None] = None) -> Tensor:
    """Resample every row of real x [.., T] to ceil(T up / down) samples with a zero-phase low-pass FIR: the Kaiser (beta 5) design of
    20 max(up, down) + 1 taps, or the caller's taps (scipy's window=array).  scipy.signal.resample_poly(x, up, down, axis=-1)."""
    return Tensor(B.dsc_resample_poly(_get_ctx(), x._c_ptr, int(up), int(down), _c_ptr_or_none(taps), _c_ptr_or_none(out)), out is not None)


def decimate(x: Tensor, q: int, n: Union[int, None] = None, out: Union[Tensor, None] = None) -> Tensor:
    """Low-pass (Hamming FIR of order n, default 20 q) and keep every q-th sample, zero phase.
    scipy.signal.decimate(x, q, n, ftype='fir')."""
    return Tensor(B.dsc_decimate(_get_ctx(), x._c_ptr, int(q), 0 if n is None else int(n), _c_ptr_or_none(out)), out is not None)


def firwin(numtaps: int, cutoff: float, window: str = 'hamming', beta: float = 5.0, dtype: Dtype = Dtype.F32) -> Tensor:
    """Low-pass FIR design by the window method: scipy.signal.firwin(numtaps, cutoff, window='hamming' or ('kaiser', beta)), cutoff
    as a fraction of the Nyquist frequency, unit gain at DC."""
    if window not in _FIRWIN_WINDOWS:
        raise ValueError(f"firwin: window must be 'hamming' or 'kaiser', got {window!r}")
    return Tensor(B.dsc_firwin(_get_ctx(), int(numtaps), float(cutoff), _FIRWIN_WINDOWS[window], float(beta), dtype.value))


def filter_fft(s: Tensor, H: Tensor, out=None) -> Tensor:
    """irfft(rfft(s, n) * H) with n = 2 * (len(H) - 1), fused where a kernel exists."""
    return Tensor(B.dsc_filter_fft(_get_ctx(), s._c_ptr, H._c_ptr, _c_ptr_or_none(out)), out is not None)


def transpose(x: Tensor, axes=None) -> Tensor:                            # python/dsc/tensor.py:407-416
    if axes is None or (isinstance(axes, (tuple, list)) and all(isinstance(a, int) for a in axes)):
        return Tensor(B.dsc_transpose(_get_ctx(), x._c_ptr, *(tuple(axes) if axes is not None else ())))
    raise RuntimeError(f'cannot transpose axes {axes}')


def fftfreq(n: int, d: float = 1.0, dtype: Dtype = Dtype.F32) -> Tensor:   # python/dsc/tensor.py:729-730
    return Tensor(B.dsc_fftfreq(_get_ctx(), n, d, dtype.value))


def rfftfreq(n: int, d: float = 1.0, dtype: Dtype = Dtype.F32) -> Tensor:  # python/dsc/tensor.py:733-734
    return Tensor(B.dsc_rfftfreq(_get_ctx(), n, d, dtype.value))


# ---- short-time transforms (include/dsc_mi355x.h, Section D) -------------------------------------------------------------------
# torch.stft / torch.istft semantics (onesided, normalized=False, win_length == n_fft) with a FRAMES-MAJOR spectrum
# [.., n_frames, n_fft // 2 + 1] = torch.stft(...).transpose(-2, -1).  Arguments are checked here and raise ValueError, so that
# the C library's print-and-exit is never reached from Python.

def _check_stft_args(n_fft: int, hop_length, window, real_dtype: Dtype) -> int:
    if not isinstance(n_fft, (int, np.integer)) or n_fft < 4 or n_fft > (1 << 20) or n_fft & (n_fft - 1):
        raise ValueError(f'n_fft must be a power of two in [4, 2^20], got {n_fft}')
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    if hop < 1:
        raise ValueError(f'hop_length must be >= 1, got {hop}')
    if window is not None:
        if not isinstance(window, Tensor) or window.n_dim != 1 or len(window) != n_fft:
            raise ValueError(f'window must be a 1-D Tensor of n_fft = {n_fft} elements')
        if window.dtype != real_dtype:
            raise ValueError(f'window dtype {window.dtype} does not match the transform precision {real_dtype}')
    return hop


_INT_MAX = 0x7fffffff                      # a tensor holds at most this many elements (`int ne`)


def _check_out(out, shape, dtype: Dtype, what: str):
    if out is not None and (not isinstance(out, Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype):
        got = (tuple(out.shape), out.dtype) if isinstance(out, Tensor) else type(out).__name__
        raise ValueError(f'{what}: out must be a {dtype} Tensor of shape {tuple(shape)}, got {got}')


def stft_n_frames(T: int, n_fft: int, hop_length: int, center: bool = True) -> int:
    """Frames of a length-T signal: 1 + T // hop with center, 1 + (T - n_fft) // hop without."""
    return 1 + T // hop_length if center else 1 + (T - n_fft) // hop_length


def stft(x: Tensor, n_fft: int, hop_length: Union[int, None] = None, window: Union[Tensor, None] = None, center: bool = True,
         pad_mode: str = 'reflect', out: Union[Tensor, None] = None) -> Tensor:
    """Short-time Fourier transform of real x [.., T] (at most 3 dims) -> complex [.., n_frames, n_fft // 2 + 1] (frames-major:
    torch.stft(...).transpose(-2, -1)).  hop_length defaults to n_fft // 4; window None = rectangular; pad_mode 'reflect' or
    'constant' (zeros), used with center only."""
    if x.dtype not in (Dtype.F32, Dtype.F64):
        raise ValueError(f'stft input must be real (f32 / f64), got {x.dtype}')
    if not 1 <= x.n_dim <= 3:
        raise ValueError(f'stft input has 1 to 3 dimensions, got {x.n_dim}')
    hop = _check_stft_args(n_fft, hop_length, window, x.dtype)
    if pad_mode not in ('reflect', 'constant'):
        raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
    T = x.shape[-1]
    if center and pad_mode == 'reflect' and T <= n_fft // 2:
        raise ValueError(f'reflect padding needs T > n_fft // 2 (T = {T}, n_fft = {n_fft})')
    if not center and T < n_fft:
        raise ValueError(f'without center the signal needs T >= n_fft (T = {T}, n_fft = {n_fft})')
    n_frames = stft_n_frames(T, n_fft, hop, center)
    shape = tuple(x.shape[:-1]) + (n_frames, n_fft // 2 + 1)
    if int(np.prod(shape, dtype=np.int64)) > _INT_MAX:
        raise ValueError(f'stft output {shape} has more than 2^31 - 1 elements')
    _check_out(out, shape, Dtype.C32 if x.dtype == Dtype.F32 else Dtype.C64, 'stft')
    return Tensor(B.dsc_stft(_get_ctx(), x._c_ptr, n_fft, hop, _c_ptr_or_none(window), bool(center), 0 if pad_mode == 'reflect' else 1,
                             _c_ptr_or_none(out)), out is not None)


def _nola_min(w2: np.ndarray, n_fft: int, hop: int, n_frames: int, start: int, end: int) -> float:
    """Smallest squared-window envelope over padded output positions [start, end) (end clipped to the last frame's end); inf if
    the range is empty.  O(n_fft + hop) host work, the same numbers in the same order as nola_min in dsc_amd/csrc/stft.cpp: with
    W[k, r] = w2[r + k hop] (zero past n_fft), position p = q hop + r sums W[k, r] over k in [max(0, q - n_frames + 1),
    min(K - 1, q)] — prefix sums down column r (suffix sums where the range reaches the last row) — and positions more than
    (K + 1) hop from both ends all see the full column sum, so one period of them stands for the rest.
    (builtins.min: this module defines its own min / max / sum.)"""
    end = builtins.min(end, n_fft + hop * (n_frames - 1))
    if end <= start:
        return float('inf')
    K = -(-n_fft // hop)
    W = np.zeros(K * hop)
    W[:n_fft] = w2
    W = W.reshape(K, hop)
    pre = np.concatenate([np.zeros((1, hop)), np.cumsum(W, axis=0)])                 # pre[k] = rows < k
    suf = np.concatenate([np.cumsum(W[::-1], axis=0)[::-1], np.zeros((1, hop))])      # suf[k] = rows >= k

    def env(p):
        q, r = p // hop, p % hop
        lo, hi = np.maximum(0, q - n_frames + 1), np.minimum(K - 1, q)
        e = np.where(lo == 0, pre[hi + 1, r], np.where(hi == K - 1, suf[lo, r], pre[hi + 1, r] - pre[lo, r]))
        return np.where(hi < lo, 0.0, e)

    span = (K + 1) * hop
    h_end = builtins.min(end, start + span)
    t_start = builtins.max(h_end, end - span)
    best = float(env(np.arange(start, h_end, dtype=np.int64)).min())
    if t_start < end:
        best = builtins.min(best, float(env(np.arange(t_start, end, dtype=np.int64)).min()))
    if h_end < t_start:
        best = builtins.min(best, float(suf[0, np.arange(h_end, builtins.min(t_start, h_end + hop)) % hop].min()))
    return best


def istft(X: Tensor, n_fft: int, hop_length: Union[int, None] = None, window: Union[Tensor, None] = None, center: bool = True,
          length: Union[int, None] = None, out: Union[Tensor, None] = None) -> Tensor:
    """Inverse of stft: complex X [.., n_frames, n_fft // 2 + 1] -> real [.., length] (torch.istft semantics).  length None = the
    natural length; samples past the last frame are zero.  Raises ValueError when the window violates NOLA (squared-window
    envelope < 1e-11 where the output is read); that check copies the window to the host (synchronous)."""
    if X.dtype not in (Dtype.C32, Dtype.C64):
        raise ValueError(f'istft input must be complex (c32 / c64), got {X.dtype}')
    if not 2 <= X.n_dim <= 4:
        raise ValueError(f'istft input must be [.., n_frames, n_fft // 2 + 1], got {X.n_dim} dimensions')
    real_dtype = Dtype.F32 if X.dtype == Dtype.C32 else Dtype.F64
    hop = _check_stft_args(n_fft, hop_length, window, real_dtype)
    n_frames, bins = X.shape[-2], X.shape[-1]
    if bins != n_fft // 2 + 1:
        raise ValueError(f'istft input has {bins} bins, n_fft = {n_fft} needs {n_fft // 2 + 1}')
    pad = n_fft // 2 if center else 0
    natural = hop * (n_frames - 1) + (0 if center else n_fft)
    n_out = natural if length is None or length <= 0 else int(length)
    if n_out < 1:
        raise ValueError(f'istft output length {n_out} < 1')
    shape = tuple(X.shape[:-2]) + (n_out,)
    if int(np.prod(shape, dtype=np.int64)) > _INT_MAX:
        raise ValueError(f'istft output {shape} has more than 2^31 - 1 elements')
    _check_out(out, shape, real_dtype, 'istft')
    w2 = np.ones(n_fft) if window is None else window.numpy().astype(np.float64) ** 2
    env_min = _nola_min(w2, n_fft, hop, n_frames, pad, pad + n_out)
    if not env_min >= 1e-11:
        raise ValueError(f'window overlap-add envelope {env_min:.3g} < 1e-11: the window / hop violate NOLA')
    return Tensor(B.dsc_istft(_get_ctx(), X._c_ptr, n_fft, hop, _c_ptr_or_none(window), bool(center), n_out, _c_ptr_or_none(out)),
                  out is not None)


# ---- linear convolution (include/dsc_mi355x.h, Section E) ------------------------------------------------------------------------
# Row r of the result = np.convolve(x[r], h, 'full')[n0 : n0 + T_out], n0 = 0 / (M - 1) // 2 / M - 1 for full / same / valid: numpy's
# convolve / correlate along the last axis whenever M <= T, scipy.signal.fftconvolve(x, h[None], mode, axes=-1) always.
_CONV_MODES = {'full': 0, 'same': 1, 'valid': 2}


def _conv(fn, what: str, x: Tensor, h: Tensor, mode: str, out) -> Tensor:
    if not isinstance(x, Tensor) or not isinstance(h, Tensor):
        raise ValueError(f'{what}: x and h must be Tensors')
    if x.dtype not in (Dtype.F32, Dtype.F64) or h.dtype not in (Dtype.F32, Dtype.F64):
        raise ValueError(f'{what}: inputs must be real (f32 / f64), got {x.dtype} and {h.dtype}')
    if h.dtype != x.dtype:
        raise ValueError(f'{what}: x and h must have the same dtype, got {x.dtype} and {h.dtype}')
    if not 1 <= x.n_dim <= 3:
        raise ValueError(f'{what}: x has 1 to 3 dimensions, got {x.n_dim}')
    if h.n_dim != 1 or h.ne < 1:
        raise ValueError(f'{what}: h must be 1-D with at least one tap, got shape {h.shape}')
    if mode not in _CONV_MODES:
        raise ValueError(f"{what}: mode must be 'full', 'same' or 'valid', got {mode!r}")
    T, M = x.shape[-1], h.ne
    if mode == 'valid' and M > T:
        raise ValueError(f'{what}: valid mode needs len(h) <= T (M = {M}, T = {T})')
    T_out = {'full': T + M - 1, 'same': T, 'valid': T - M + 1}[mode]
    shape = tuple(x.shape[:-1]) + (T_out,)
    if int(np.prod(shape, dtype=np.int64)) > _INT_MAX:
        raise ValueError(f'{what}: output {shape} has more than 2^31 - 1 elements')
    _check_out(out, shape, x.dtype, what)
    if out is not None:
        es = np.dtype(DTYPE_TO_NP[x.dtype]).itemsize
        xa, oa = x._c_ptr.contents.data, out._c_ptr.contents.data
        if oa < xa + x.ne * es and xa < oa + out.ne * es:
            raise ValueError(f'{what}: out must not share memory with x')
    return Tensor(fn(_get_ctx(), x._c_ptr, h._c_ptr, _CONV_MODES[mode], _c_ptr_or_none(out)), out is not None)


def convolve(x: Tensor, h: Tensor, mode: str = 'full', out: Union[Tensor, None] = None) -> Tensor:
    """Linear convolution of every row of real x [.., T] (at most 3 dims) with real h [M] of the same dtype: mode 'full'
    (T + M - 1 samples), 'same' (T) or 'valid' (T - M + 1, needs M <= T).  numpy.convolve along the last axis."""
    return _conv(B.dsc_convolve, 'convolve', x, h, mode, out)


def correlate(x: Tensor, h: Tensor, mode: str = 'valid', out: Union[Tensor, None] = None) -> Tensor:
    """numpy.correlate along the last axis for real inputs: convolve with h reversed."""
    return _conv(B.dsc_correlate, 'correlate', x, h, mode, out)


# ---- windows (torch's definitions; computed on the host in f64, then uploaded) ---------------------------------------------------
def _window(values: np.ndarray, dtype: Dtype) -> Tensor:
    if dtype not in (Dtype.F32, Dtype.F64):
        raise ValueError(f'window dtype must be f32 or f64, got {dtype}')
    return from_numpy(values.astype(DTYPE_TO_NP[dtype]))


def _cosine_sum(n: int, periodic: bool, coeffs) -> np.ndarray:
    if n < 0:
        raise ValueError(f'window length must be >= 0, got {n}')
    if n == 1:
        return np.ones(1)
    m = n if periodic else n - 1
    k = np.arange(n, dtype=np.float64)
    return np.sum([(-1) ** i * a * np.cos(2.0 * np.pi * i * k / m) for i, a in enumerate(coeffs)], axis=0)


def hann_window(n: int, periodic: bool = True, dtype: Dtype = Dtype.F32) -> Tensor:
    """torch.hann_window: 0.5 - 0.5 cos(2 pi k / N), N = n (periodic) or n - 1."""
    return _window(_cosine_sum(n, periodic, (0.5, 0.5)), dtype)


def hamming_window(n: int, periodic: bool = True, dtype: Dtype = Dtype.F32) -> Tensor:
    """torch.hamming_window: 0.54 - 0.46 cos(2 pi k / N)."""
    return _window(_cosine_sum(n, periodic, (0.54, 0.46)), dtype)


def blackman_window(n: int, periodic: bool = True, dtype: Dtype = Dtype.F32) -> Tensor:
    """torch.blackman_window: 0.42 - 0.5 cos(2 pi k / N) + 0.08 cos(4 pi k / N)."""
    return _window(_cosine_sum(n, periodic, (0.42, 0.5, 0.08)), dtype)


def kaiser_window(n: int, periodic: bool = True, beta: float = 12.0, dtype: Dtype = Dtype.F32) -> Tensor:
    """torch.kaiser_window: I0(beta sqrt(1 - (2 k / N - 1)^2)) / I0(beta), N = n (periodic) or n - 1."""
    if n < 0:
        raise ValueError(f'window length must be >= 0, got {n}')
    if n == 1:
        return _window(np.ones(1), dtype)
    m = n if periodic else n - 1
    k = np.arange(n, dtype=np.float64)
    return _window(np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * k / m - 1.0) ** 2))) / np.i0(beta), dtype)
