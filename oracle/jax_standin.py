"""A narrow stand-in for the part of JAX that the reference's loss path calls, built on torch float64 + autograd.

TEST INFRASTRUCTURE ONLY, and only for ``tests/golden/make_reference_golden.py``: it lets the reference's own
(unmodified) modules run on a machine without jax, so that what they compute can be recorded as fixtures.  Nothing
in the package, the oracle, a ``conftest.py`` or a test of the engine installs it; ``install()`` is called by the
recorder alone, in its own process.

Written from JAX's documented semantics with ``jax_enable_x64`` on (the reference runs in float64).  Arrays are
``Array`` objects wrapping a ``torch.Tensor`` (float64 by default, int64 for Python ints), so torch autograd through
them gives what ``jax.value_and_grad`` would.  Only what the recorded functions call is implemented; anything else
raises.  The places where a naive mapping to torch would be wrong carry a comment, and each is tested in
``tests/test_jax_standin.py``:

  J1  ``.at[idx].add(v, mode='drop')``: negative indices in [-n, -1] are normalised (+n) first, and only then are
      out-of-range updates dropped ("wrap-then-drop"); duplicates accumulate.
  J2  ``.at[idx].set(v, mode='drop')`` with repeated indices: one update wins (the last here) and only the winner
      receives a cotangent.  torch's ``index_put`` would send the cotangent to every duplicate.
  J3  ``min``/``max`` reductions share the cotangent equally among tied elements (``torch.amin``/``amax``).
  J4  ``abs'(0) = 0``.
  J5  ``jnp.round`` rounds half to even; ``astype(int)`` truncates toward zero.
  J6  ``jax.scipy.signal.convolve(a, k, mode='same')`` is a true convolution (kernel flipped), zero padded, centred
      like ``scipy.signal.convolve``.  Three summation modes (``set_convolve_mode``): ``taps`` (ordered sum of
      shifted products), ``reversed`` (the same taps in reverse order) and ``exact`` (forward values are the exact
      sum rounded once to float64; the gradient is the same linear map's adjoint).
  J7  ``jax.scipy.stats.multivariate_normal.pdf``: the general Cholesky formula.
  J8  ``jax.image.scale_and_translate``: separable per-axis weight matrices (triangle, Keys cubic a=-0.5,
      Lanczos 3/5), antialias widening only when downscaling, weights normalised by their sum and zeroed where that
      sum is ~0 or the sample lies outside the input.
  J9  ``jnp.var`` is the population variance.
  J10 ``jax.vmap`` loops over the mapped axis and stacks (tuples of outputs included); ``jnp.array(list)`` stacks.
  J11 Type promotion: int combined with a Python float or a float array gives float64; int32 with int64 gives int64.
"""
import math
import sys
import types

import numpy as np
import torch

F64 = torch.float64

_DTYPES = {
    'float64': torch.float64, 'float32': torch.float32, 'int64': torch.int64, 'int32': torch.int32,
    'int16': torch.int16, 'int8': torch.int8, 'uint8': torch.uint8, 'bool': torch.bool,
}


def _torch_dtype(d):
    if isinstance(d, torch.dtype):
        return d
    if d is float:
        return torch.float64
    if d is int:
        return torch.int64
    if d is bool:
        return torch.bool
    return _DTYPES[np.dtype(d).name]


def _t(x):
    """Anything array-like -> torch.Tensor (Python ints -> int64, floats -> float64, J11)."""
    if isinstance(x, Array):
        return x.t
    if isinstance(x, torch.Tensor):
        return x
    if isinstance(x, np.ndarray) or isinstance(x, np.generic):
        return torch.from_numpy(np.array(x, copy=True))
    if isinstance(x, (list, tuple)):
        if any(isinstance(e, (Array, torch.Tensor, np.ndarray)) for e in x):
            return torch.stack([_t(e) for e in x])                          # J10: jnp.array(list_of_arrays) stacks
        a = np.array(x)
        if a.dtype.kind == 'f':
            a = a.astype(np.float64)
        return torch.from_numpy(a)
    if isinstance(x, bool):
        return torch.tensor(x)
    if isinstance(x, int):
        return torch.tensor(x, dtype=torch.int64)
    if isinstance(x, float):
        return torch.tensor(x, dtype=F64)
    raise TypeError(f'jax stand-in: cannot make an array from {type(x).__name__}')


def _promote(a, b):
    """J11: bring an int/bool tensor to float64 when the other operand is floating (a Python float included)."""
    ta = a.t if isinstance(a, Array) else a
    tb = b.t if isinstance(b, Array) else b
    if isinstance(ta, np.ndarray) or isinstance(ta, np.generic):
        ta = _t(ta)
    if isinstance(tb, np.ndarray) or isinstance(tb, np.generic):
        tb = _t(tb)

    def is_float(v):
        return (isinstance(v, torch.Tensor) and v.is_floating_point()) or isinstance(v, float)

    if is_float(ta) and isinstance(tb, torch.Tensor) and not tb.is_floating_point():
        tb = tb.to(F64)
    if is_float(tb) and isinstance(ta, torch.Tensor) and not ta.is_floating_point():
        ta = ta.to(F64)
    return ta, tb


def _wrap(v):
    return Array(v) if isinstance(v, torch.Tensor) else v


def _index(idx):
    """Index for a gather: Arrays -> long tensors (torch will not index with int16)."""
    def one(i):
        if isinstance(i, (Array, np.ndarray, torch.Tensor)):
            t = _t(i)
            return t if t.dtype == torch.bool else t.long()
        return i
    return tuple(one(i) for i in idx) if isinstance(idx, tuple) else one(idx)


class _At:
    def __init__(self, arr):
        self.arr = arr

    def __getitem__(self, idx):
        return _AtIndex(self.arr, idx if isinstance(idx, tuple) else (idx,))


class _AtIndex:
    def __init__(self, arr, idx):
        self.arr, self.idx = arr, idx

    def _normalised(self, mode):
        if mode != 'drop':
            raise NotImplementedError("jax stand-in: only mode='drop' scatters are used")
        base = self.arr.t
        if len(self.idx) != base.dim():
            raise NotImplementedError('jax stand-in: a scatter must index every axis')
        parts = [_t(i).long() if not isinstance(i, int) else torch.tensor(i, dtype=torch.int64) for i in self.idx]
        parts = torch.broadcast_tensors(*parts)
        valid = torch.ones(parts[0].shape, dtype=torch.bool)
        out = []
        for p, n in zip(parts, base.shape):
            p = torch.where(p < 0, p + n, p)          # J1: wrap first: [-n, -1] -> [0, n-1] ...
            valid &= (p >= 0) & (p < n)               # ... then drop what is still out of range
            out.append(p)
        return base, out, valid

    def add(self, v, mode=None):
        base, parts, valid = self._normalised(mode)
        tb, tv = _promote(Array(base), v)
        tv = torch.broadcast_to(tv.to(tb.dtype), parts[0].shape)
        return Array(tb.index_put(tuple(p[valid] for p in parts), tv[valid], accumulate=True))

    def set(self, v, mode=None):
        base, parts, valid = self._normalised(mode)
        tv = _t(v) if not isinstance(v, (int, float, bool)) else torch.tensor(v)
        tv = torch.broadcast_to(tv.to(base.dtype), parts[0].shape)[valid]
        parts = [p[valid] for p in parts]
        # J2: with repeated indices exactly one update lands and only it gets a cotangent.  Keep the last occurrence of
        # every linear index before index_put, which would otherwise route the cotangent to all duplicates.
        lin = torch.zeros_like(parts[0])
        for p, n in zip(parts, base.shape):
            lin = lin * n + p
        if lin.numel():
            uniq, inv = torch.unique(lin, return_inverse=True)
            pos = torch.arange(lin.numel())
            last = torch.full((uniq.numel(),), -1, dtype=torch.int64).scatter_reduce(0, inv, pos, reduce='amax')
            parts = [p[last] for p in parts]
            tv = tv[last]
        return Array(base.index_put(tuple(parts), tv, accumulate=False))


class Array:
    """A JAX-array look-alike over a torch tensor."""
    __array_priority__ = 1000          # ndarray (op) Array defers to Array's reflected operators

    def __init__(self, t):
        self.t = t

    # -- metadata ---------------------------------------------------------------------------------
    @property
    def shape(self):
        return tuple(self.t.shape)

    @property
    def ndim(self):
        return self.t.dim()

    @property
    def size(self):
        return self.t.numel()

    @property
    def dtype(self):
        return np.dtype(str(self.t.dtype).replace('torch.', ''))

    @property
    def T(self):
        return Array(self.t.permute(*reversed(range(self.t.dim()))))

    @property
    def at(self):
        return _At(self)

    def __len__(self):
        return self.t.shape[0]

    def __iter__(self):
        return (Array(self.t[i]) for i in range(self.t.shape[0]))

    def __repr__(self):
        return f'Array({self.t!r})'

    def __array__(self, dtype=None):
        a = self.t.detach().numpy()
        return a.astype(dtype) if dtype is not None else a

    def __float__(self):
        return float(self.t)

    def __int__(self):
        return int(self.t)

    def __bool__(self):
        return bool(self.t)

    def tolist(self):
        return self.t.tolist()

    # -- shape ------------------------------------------------------------------------------------
    def __getitem__(self, idx):
        return Array(self.t[_index(idx)])

    def transpose(self, *axes):
        if len(axes) == 1 and isinstance(axes[0], (tuple, list)):
            axes = tuple(axes[0])
        if not axes:
            axes = tuple(reversed(range(self.t.dim())))
        return Array(self.t.permute(*axes))        # numpy-style transpose(2, 0, 1)

    def reshape(self, *shape):
        return Array(self.t.reshape(*shape))

    def astype(self, dtype):
        d = _torch_dtype(dtype)
        if self.t.is_floating_point() and not d.is_floating_point and d != torch.bool:
            return Array(torch.trunc(self.t).to(d))  # J5: float -> int truncates toward zero
        return Array(self.t.to(d))

    # -- reductions -------------------------------------------------------------------------------
    def sum(self, axis=None):
        return sum_(self, axis)

    def mean(self, axis=None):
        return mean(self, axis)

    def min(self, axis=None):
        return min_(self, axis)

    def max(self, axis=None):
        return max_(self, axis)

    def var(self, axis=None):
        return var(self, axis)

    # -- arithmetic -------------------------------------------------------------------------------
    def _bin(self, other, op, reflected=False):
        a, b = _promote(self, other)
        return _wrap(op(b, a) if reflected else op(a, b))

    def __add__(self, o): return self._bin(o, torch.add)
    def __radd__(self, o): return self._bin(o, torch.add, True)
    def __sub__(self, o): return self._bin(o, torch.sub)
    def __rsub__(self, o): return self._bin(o, torch.sub, True)
    def __mul__(self, o): return self._bin(o, torch.mul)
    def __rmul__(self, o): return self._bin(o, torch.mul, True)
    def __truediv__(self, o): return self._bin(o, _true_div)
    def __rtruediv__(self, o): return self._bin(o, _true_div, True)
    def __pow__(self, o): return self._bin(o, torch.pow)
    def __neg__(self): return Array(-self.t)
    def __gt__(self, o): return self._bin(o, torch.gt)
    def __ge__(self, o): return self._bin(o, torch.ge)
    def __lt__(self, o): return self._bin(o, torch.lt)
    def __le__(self, o): return self._bin(o, torch.le)
    def __eq__(self, o): return self._bin(o, torch.eq)
    def __ne__(self, o): return self._bin(o, torch.ne)
    def __or__(self, o): return self._bin(o, torch.bitwise_or)
    def __and__(self, o): return self._bin(o, torch.bitwise_and)
    def __invert__(self): return Array(~self.t)
    __hash__ = None


def _true_div(a, b):
    if isinstance(a, torch.Tensor) and not a.is_floating_point():
        a = a.to(F64)
    if isinstance(b, torch.Tensor) and not b.is_floating_point():
        b = b.to(F64)
    return a / b


# ------------------------------------------------------------------------------------------------------
# jax.numpy
# ------------------------------------------------------------------------------------------------------
def array(x, dtype=None):
    t = _t(x)
    return Array(t.to(_torch_dtype(dtype)) if dtype is not None else t)


def zeros(shape, dtype=None):
    shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
    return Array(torch.zeros(shape, dtype=_torch_dtype(dtype) if dtype is not None else F64))


def ones_like(a, dtype=None):
    t = _t(a)
    return Array(torch.ones_like(t, dtype=_torch_dtype(dtype) if dtype is not None else t.dtype))


def round(a, decimals=0):  # noqa: A001 - jnp.round
    if decimals != 0:
        raise NotImplementedError('jax stand-in: round with decimals')
    t = _t(a)
    # J5: torch.round is round-half-to-even like jnp.round; integers pass through unchanged
    return Array(torch.round(t) if t.is_floating_point() else t)


def abs(a):  # noqa: A001 - jnp.abs
    return Array(torch.abs(_t(a)))           # J4: torch's abs has derivative sign(0) = 0 at 0, as JAX's


def _axis(axis):
    return tuple(axis) if isinstance(axis, (tuple, list)) else axis


def sum_(a, axis=None):
    t = _t(a)
    if t.dtype == torch.bool:
        t = t.long()
    return Array(t.sum() if axis is None else t.sum(dim=_axis(axis)))


def mean(a, axis=None):
    t = _promote(a, 1.0)[0]
    return Array(t.mean() if axis is None else t.mean(dim=_axis(axis)))


def min_(a, axis=None):
    t = _t(a)
    return Array(torch.amin(t) if axis is None else torch.amin(t, dim=_axis(axis)))  # J3: ties share the cotangent


def max_(a, axis=None):
    t = _t(a)
    return Array(torch.amax(t) if axis is None else torch.amax(t, dim=_axis(axis)))  # J3


def var(a, axis=None):
    # J9: population variance, two-pass as jnp.var: mean((a - mean(a))**2)
    t = _promote(a, 1.0)[0]
    if axis is None:
        c = t - t.mean()
        return Array((c * c).mean())
    c = t - t.mean(dim=_axis(axis), keepdim=True)
    return Array((c * c).mean(dim=_axis(axis)))


def stack(arrays, axis=0):
    ts = [_t(a) for a in arrays]
    dt = ts[0].dtype
    for t in ts[1:]:
        dt = torch.promote_types(dt, t.dtype)
    return Array(torch.stack([t.to(dt) for t in ts], dim=axis))


# ------------------------------------------------------------------------------------------------------
# jax.scipy.signal.convolve (J6)
# ------------------------------------------------------------------------------------------------------
CONVOLVE_MODES = ('taps', 'reversed', 'exact')
_convolve_mode = ['exact']


def set_convolve_mode(mode):
    if mode not in CONVOLVE_MODES:
        raise ValueError(f'convolve mode {mode!r}: one of {CONVOLVE_MODES}')
    _convolve_mode[0] = mode


def get_convolve_mode():
    return _convolve_mode[0]


def _conv_taps(x, k):
    """'same' true convolution as a list of (kernel entry, shifted input) taps, in kernel-raster order.

    full[y] = sum_a k[a] x[y - a]; 'same' keeps full[y + (kh - 1)//2] (scipy.signal.convolve's centring), so tap (a, b)
    reads x[y + ch - a, x + cw - b] with zero padding, ch = (kh - 1)//2, cw = (kw - 1)//2.
    """
    H, W = x.shape
    kh, kw = k.shape
    ch, cw = (kh - 1) // 2, (kw - 1) // 2
    pad = torch.nn.functional.pad(x, (kw, kw, kh, kh))       # wide enough for every shift
    taps = []
    for a in range(kh):
        for b in range(kw):
            dy, dx = ch - a, cw - b
            taps.append((a, b, pad[kh + dy:kh + dy + H, kw + dx:kw + dx + W]))
    return taps


def _two_prod(a, b):
    """Error-free product a*b = p + e (Dekker / Veltkamp splitting; float64, no overflow)."""
    p = a * b
    c = 134217729.0                         # 2**27 + 1
    t = c * a; ah = t - (t - a); al = a - ah
    t = c * b; bh = t - (t - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_convolve_values(x, k):
    """The exact 'same' convolution of float64 x with float64 k, rounded once to float64 (numpy in, numpy out).

    Each product is split exactly into p + e, and math.fsum returns the correctly rounded sum of all of them, so the
    result is independent of any summation order (tests/test_jax_standin.py checks it against fractions.Fraction).
    """
    x = np.asarray(x, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    terms = []
    for a, b, s in _conv_taps(torch.from_numpy(x), torch.from_numpy(k)):
        p, e = _two_prod(np.full(s.shape, k[a, b]), s.numpy())
        terms.append(p)
        terms.append(e)
    rows = np.stack(terms).reshape(len(terms), -1).T.tolist()
    return np.array([math.fsum(r) for r in rows], dtype=np.float64).reshape(x.shape)


def convolve(in1, in2, mode='full', method='auto', precision=None):
    if mode != 'same':
        raise NotImplementedError("jax stand-in: only convolve(..., mode='same')")
    x, k = _t(in1), _t(in2)
    x = x if x.is_floating_point() else x.to(F64)
    k = k.to(F64)
    if x.dim() != 2 or k.dim() != 2:
        raise NotImplementedError('jax stand-in: 2-D convolve only')
    taps = _conv_taps(x, k)
    m = _convolve_mode[0]
    order = reversed(taps) if m == 'reversed' else taps
    out = torch.zeros_like(x)
    for a, b, s in order:
        out = out + k[a, b] * s
    if m == 'exact':
        # forward: the exact sum rounded once; backward: the convolution's own adjoint (straight through)
        ex = torch.from_numpy(exact_convolve_values(x.detach().numpy(), k.detach().numpy()))
        out = out + (ex - out).detach()
    return Array(out)


# ------------------------------------------------------------------------------------------------------
# jax.scipy.stats.multivariate_normal.pdf (J7)
# ------------------------------------------------------------------------------------------------------
def mvn_logpdf(x, mean, cov):
    x, m, c = _promote(x, 1.0)[0], _t(mean), _t(cov)
    m = m.to(F64)
    c = c.to(F64)
    n = m.shape[-1]
    L = torch.linalg.cholesky(c)
    d = (x - m).unsqueeze(-1)
    y = torch.linalg.solve_triangular(L, d.reshape(-1, n).T, upper=False).T.reshape(x.shape)
    return -0.5 * (y * y).sum(-1) - (n / 2) * math.log(2 * math.pi) - torch.log(torch.diagonal(L)).sum()


def mvn_pdf(x, mean, cov, allow_singular=None):
    return Array(torch.exp(mvn_logpdf(x, mean, cov)))


# ------------------------------------------------------------------------------------------------------
# jax.image.scale_and_translate (J8)
# ------------------------------------------------------------------------------------------------------
def _k_triangle(x):
    return torch.clamp(1.0 - torch.abs(x), min=0.0)


def _k_keys_cubic(x):
    # Keys (1981) cubic convolution, a = -0.5; x >= 0 here
    near = ((1.5 * x - 2.5) * x) * x + 1.0
    far = ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0
    out = torch.where(x >= 1.0, far, near)
    return torch.where(x >= 2.0, torch.zeros_like(x), out)


def _k_lanczos(radius):
    def k(x):
        y = radius * torch.sin(math.pi * x) * torch.sin(math.pi * x / radius)
        safe = torch.where(x != 0, (math.pi ** 2) * x * x, torch.ones_like(x))
        out = torch.where(x > 1e-3, y / safe, torch.ones_like(x))
        return torch.where(x > radius, torch.zeros_like(x), out)
    return k


RESIZE_KERNELS = {
    'linear': _k_triangle, 'bilinear': _k_triangle, 'trilinear': _k_triangle, 'triangle': _k_triangle,
    'cubic': _k_keys_cubic, 'bicubic': _k_keys_cubic, 'tricubic': _k_keys_cubic,
    'lanczos3': _k_lanczos(3.0), 'lanczos5': _k_lanczos(5.0),
}


def scale_translate_weights(n_in, n_out, scale, translation, method, antialias=True):
    """(n_out, n_in) float64 matrix W with out = W @ in along one axis."""
    kernel = RESIZE_KERNELS[method]
    inv = 1.0 / scale
    widen = max(inv, 1.0) if antialias else 1.0           # antialias widens the kernel only when downscaling
    pos = (torch.arange(n_out, dtype=F64) + 0.5) * inv - translation * inv - 0.5   # sample position in input pixels
    dist = torch.abs(pos[None, :] - torch.arange(n_in, dtype=F64)[:, None]) / widen
    w = kernel(dist)                                      # (n_in, n_out)
    tot = w.sum(dim=0, keepdim=True)
    ok = torch.abs(tot) > 1000.0 * float(np.finfo(np.float32).eps)
    w = torch.where(ok, w / torch.where(tot != 0, tot, torch.ones_like(tot)), torch.zeros_like(w))
    inside = (pos >= -0.5) & (pos <= n_in - 0.5)          # samples outside the input get no weight
    w = torch.where(inside[None, :], w, torch.zeros_like(w))
    return w.T.contiguous()


def scale_and_translate(image, shape, spatial_dims, scale, translation, method, antialias=True, precision=None):
    x = _promote(image, 1.0)[0]
    sc = [float(v) for v in _t(scale).tolist()]
    tr = [float(v) for v in _t(translation).tolist()]
    out = x
    for i, d in enumerate(spatial_dims):
        Wm = scale_translate_weights(x.shape[d], shape[d], sc[i], tr[i], method, antialias)
        out = torch.movedim(torch.tensordot(Wm, torch.movedim(out, d, 0), dims=([1], [0])), 0, d)
    return Array(out)


# ------------------------------------------------------------------------------------------------------
# transformations
# ------------------------------------------------------------------------------------------------------
def jit(fun=None, **kw):
    if fun is None:
        return lambda f: f
    return fun


def vmap(fun, in_axes=0, out_axes=0):
    """J10: loop over the mapped axis and stack the outputs (tuples of outputs stacked element-wise)."""
    def mapped(*args):
        axes = in_axes if isinstance(in_axes, (tuple, list)) else (in_axes,) * len(args)
        sizes = {_t(a).shape[ax] for a, ax in zip(args, axes) if ax is not None}
        if len(sizes) != 1:
            raise ValueError('jax stand-in vmap: mapped axes must agree')
        n = sizes.pop()
        outs = []
        for i in range(n):
            call = [a if ax is None else Array(torch.select(_t(a), ax, i)) for a, ax in zip(args, axes)]
            outs.append(fun(*call))
        if isinstance(outs[0], tuple):
            return tuple(stack([o[j] for o in outs]) for j in range(len(outs[0])))
        return stack(outs)
    return mapped


# ------------------------------------------------------------------------------------------------------
# install
# ------------------------------------------------------------------------------------------------------
class _NoCV2(types.ModuleType):
    def __getattr__(self, name):
        raise RuntimeError(f'cv2.{name}: OpenCV is not part of the recorded path')


def install():
    """Put jax, jax.numpy, jax.scipy(.signal/.stats), jax.image, jax.typing and a failing cv2 into sys.modules."""
    jax = types.ModuleType('jax')
    jnp = types.ModuleType('jax.numpy')
    jsp = types.ModuleType('jax.scipy')
    sig = types.ModuleType('jax.scipy.signal')
    stats = types.ModuleType('jax.scipy.stats')
    mvn = types.ModuleType('jax.scipy.stats.multivariate_normal')
    image = types.ModuleType('jax.image')
    typing_ = types.ModuleType('jax.typing')

    jax.jit, jax.vmap, jax.Array = jit, vmap, Array
    jax.numpy, jax.scipy, jax.image, jax.typing = jnp, jsp, image, typing_
    typing_.ArrayLike = Array
    for name in ('array', 'zeros', 'ones_like', 'round', 'abs', 'mean', 'var', 'stack'):
        setattr(jnp, name, globals()[name])
    jnp.sum, jnp.min, jnp.max = sum_, min_, max_
    jnp.float64, jnp.float32, jnp.int64, jnp.int32, jnp.int16 = np.float64, np.float32, np.int64, np.int32, np.int16
    jnp.bool_ = np.bool_
    jnp.ndarray = Array
    jsp.signal, jsp.stats = sig, stats
    sig.convolve = convolve
    stats.multivariate_normal = mvn
    mvn.pdf, mvn.logpdf = mvn_pdf, lambda *a, **k: Array(mvn_logpdf(*a, **k))
    image.scale_and_translate = scale_and_translate
    sys.modules.update({
        'jax': jax, 'jax.numpy': jnp, 'jax.scipy': jsp, 'jax.scipy.signal': sig, 'jax.scipy.stats': stats,
        'jax.scipy.stats.multivariate_normal': mvn, 'jax.image': image, 'jax.typing': typing_,
        'cv2': _NoCV2('cv2'),
    })
