"""Host planner of the axis operators (``NDMPS.roll`` / ``shift`` / ``correlate1d`` / ``cumsum`` / ``flip``): NumPy only.

Site ``k`` of the chain carries digit ``k`` of every axis, coarsest first (``get_factorlist``: digit ``l`` of index
``i`` on an axis is ``(i mod prod[l]) // prod[l + 1]``).  An operator that acts along one axis is therefore a
matrix-product operator (MPO) over that axis's digits: per site a core ``M_k`` of shape ``(D_k, f_k, f_k, D_{k+1})``
indexed ``[c, o, i, c']`` (left bond, output digit, input digit, right bond), ``D_0 = D_L = 1``, applied as

    Z_k[c chi + a, ravel(.. o ..), c' chi' + a'] = sum_i M_k[c, o, i, c'] X_k[a, ravel(.. i ..), a']

where the site's physical index ravels the digits of all axes in C order (``factor_arr[k]``) and only this axis's
digit changes.  The chain ``Z`` has the bonds ``D_k chi_k`` (carry-major) and decodes to the operator applied to what
``X`` decodes to; ``ndmps_lincomb_round`` with K = 1 rounds it back (csrc/axisop.hip, csrc/lincomb.hip).

* Offsets (``offsets_mpo``): ``y[o] = sum_s taps[s] x[o - s]`` is digit-wise addition of ``s`` with a carry that
  travels from site L-1 to site 0.  The bond is the set of carries that can occur: at most 2 for a single offset, at
  most 3 for a stencil except at the finest bond (``2 ceil(r / f_last) + 1`` for radius r).
* Running sum (``cumsum_mpo``): ``i <= o`` read coarse to fine is the two-state automaton eq / lt.
* Flip (``flip_mpo``): ``n - 1 - i`` reverses every digit; bond 1.

``opnorm`` bounds the operator's 2-norm; ``opnorm * norm_value`` is the absolute scale of the rounding's storage
floor (core/lincomb.py).
"""
from __future__ import annotations

import math
import numbers
import operator

import numpy as np

from .lincomb import MAX_SUMMED_BOND

MODES = ("wrap", "constant")


class AxisMPO:
    """The cores ``M_k`` (fp64, ``(D_k, f_k, f_k, D_{k+1})``) of one axis operator and the bound on its 2-norm."""

    def __init__(self, cores, opnorm):
        self.cores = [np.ascontiguousarray(c, dtype=np.float64) for c in cores]
        self.opnorm = float(opnorm)

    @property
    def bonds(self):
        """The L + 1 bonds ``D_0 .. D_L``."""
        return [int(c.shape[0]) for c in self.cores] + [int(self.cores[-1].shape[3])]

    @property
    def factors(self):
        return [int(c.shape[1]) for c in self.cores]


# ------------------------------------------------------------------------------------------------ argument checks
def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def normalize_axis(axis, ndim) -> int:
    """One axis as a non-negative int.  TypeError for a non-integer (bools and None included), numpy's AxisError
    (a ValueError) out of range."""
    if not _is_int(axis):
        raise TypeError(f"axis must be an integer, got {type(axis).__name__}")
    a = operator.index(axis)
    if not -ndim <= a < ndim:
        raise np.exceptions.AxisError(a, ndim)
    return a % ndim


def check_shift(shift) -> int:
    """TypeError unless the shift is an integer (bools refused)."""
    if not _is_int(shift):
        raise TypeError(f"shift must be an integer, got {type(shift).__name__}")
    return operator.index(shift)


def check_mode(mode) -> str:
    if mode not in MODES:
        raise ValueError(f"mode must be 'wrap' or 'constant', got {mode!r}")
    return mode


def check_taps(weights) -> np.ndarray:
    """The stencil weights as a fp64 vector.  ValueError unless they are a non-empty 1-D array of finite numbers."""
    try:
        w = np.asarray(weights, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError("weights must be a 1-D array of real numbers") from exc
    if w.ndim != 1 or w.size == 0:
        raise ValueError("weights must be a non-empty 1-D array")
    if not np.all(np.isfinite(w)):
        raise ValueError("every weight must be finite")
    return w


def check_data_axis(mode, axis, ndim) -> None:
    """ValueError for the last axis of a DCT-mode object: its digits index DCT coefficients, not voxels."""
    if mode == "DCT" and axis == ndim - 1:
        raise ValueError("DCT mode stores the last axis as DCT coefficients; axis operators act on the other axes only")


def correlate_taps(weights, origin, n) -> dict:
    """``scipy.ndimage.correlate1d``'s ``out[i] = sum_j w[j] x[i + j - len(w) // 2 - origin]`` as the offsets of
    ``offsets_mpo``: ``{len(w) // 2 + origin - j: w[j]}``.  ValueError for bad weights, an origin outside
    ``[-(len(w) // 2), (len(w) - 1) // 2]`` (scipy's rule) or a radius ``max |offset| >= n``."""
    w = check_taps(weights)
    if not _is_int(origin):
        raise TypeError(f"origin must be an integer, got {type(origin).__name__}")
    origin = operator.index(origin)
    half = w.size // 2
    if not -half <= origin <= (w.size - 1) // 2:
        raise ValueError(f"origin {origin} outside [{-half}, {(w.size - 1) // 2}]")
    taps = {half + origin - j: float(w[j]) for j in range(w.size)}
    radius = max(abs(s) for s in taps)
    if radius >= n:
        raise ValueError(f"stencil radius {radius} must be smaller than the axis length {n}")
    return taps


def check_wide_bonds(mpo_bonds, bonds) -> None:
    """ValueError when some inner widened bond ``D_k chi_k`` exceeds MAX_SUMMED_BOND (the eigen-solver's order limit)."""
    for k in range(1, len(bonds) - 1):
        wide = int(mpo_bonds[k]) * int(bonds[k])
        if wide > MAX_SUMMED_BOND:
            raise ValueError(f"bond {k}: the operator widens {bonds[k]} to {wide} > {MAX_SUMMED_BOND}, the eigen-solver's "
                             f"limit; recompress the input first (recompress(max_bond=...))")


def _factors(fs):
    f = [int(v) for v in np.asarray(fs).ravel()]
    if not f or any(v < 1 for v in f):
        raise ValueError("fs must be a non-empty list of positive factors")
    return f


# ------------------------------------------------------------------------------------------------ the operators
def _zero_mpo(f, opnorm):
    return AxisMPO([np.zeros((1, v, v, 1)) for v in f], opnorm)


def offsets_mpo(fs, taps, mode="wrap") -> AxisMPO:
    """``y[o] = sum_s taps[s] x[o - s]`` along an axis whose digits have the radices ``fs`` (coarse to fine); ``taps``
    maps integer offsets to weights.  ``mode="wrap"``: indices are taken mod n; ``"constant"``: ``x`` is 0 outside
    ``[0, n)``.

    The state on the virtual bond right of site L-1 is the offset.  At site k an incoming carry ``c'`` and input digit
    ``i`` give the output digit ``(i + c') mod f_k`` and the outgoing carry ``(i + c') // f_k`` (floor: carries may be
    negative).  The taps are contracted into the last core.  At site 0 "wrap" sums over every outgoing carry and
    "constant" keeps the carry 0; carries that cannot reach a kept one are left out of the bonds.  ``opnorm`` is
    ``sum |taps|``.  Taps of weight 0 are dropped; an operator with nothing left has bond 1 and zero cores."""
    f = _factors(fs)
    check_mode(mode)
    L = len(f)
    tp = {}
    for s, w in dict(taps).items():
        if not _is_int(s):
            raise TypeError(f"offsets must be integers, got {type(s).__name__}")
        w = float(w)
        if not math.isfinite(w):
            raise ValueError("every weight must be finite")
        if w != 0.0:
            tp[operator.index(s)] = tp.get(operator.index(s), 0.0) + w
    opnorm = sum(abs(w) for w in tp.values())
    if not tp:
        return _zero_mpo(f, opnorm)
    # forward: the carries that occur on each bond, from the finest site up (state[L] = the offsets)
    state = [None] * (L + 1)
    state[L] = sorted(tp)
    for k in range(L - 1, -1, -1):
        state[k] = sorted({(i + c) // f[k] for c in state[k + 1] for i in range(f[k])})
    # backward: keep the carries from which a kept final carry can be reached
    state[0] = list(state[0]) if mode == "wrap" else [c for c in state[0] if c == 0]
    for k in range(L):
        alive = set(state[k])
        state[k + 1] = [c for c in state[k + 1] if any((i + c) // f[k] in alive for i in range(f[k]))]
    if any(not s for s in state):
        return _zero_mpo(f, opnorm)
    cores = []
    for k in range(L):
        left = {c: j for j, c in enumerate(state[k])}
        d_left = 1 if k == 0 else len(left)  # site 0: every kept final carry lands on the one boundary state
        d_right = 1 if k == L - 1 else len(state[k + 1])
        m = np.zeros((d_left, f[k], f[k], d_right))
        for j, c in enumerate(state[k + 1]):
            for i in range(f[k]):
                out = (i + c) // f[k]
                if out in left:
                    m[0 if k == 0 else left[out], (i + c) % f[k], i, 0 if k == L - 1 else j] += tp[c] if k == L - 1 else 1.0
        cores.append(m)
    return AxisMPO(cores, opnorm)


def roll_mpo(fs, shift) -> AxisMPO:
    """``np.roll`` by ``shift`` along the axis: the single offset ``shift mod n``, periodic."""
    n = int(np.prod(_factors(fs), dtype=np.int64))
    return offsets_mpo(fs, {check_shift(shift) % n: 1.0}, "wrap")


def shift_mpo(fs, shift) -> AxisMPO:
    """The zero-filled shift: ``y[o] = x[o - shift]`` inside ``[0, n)``, 0 elsewhere."""
    return offsets_mpo(fs, {check_shift(shift): 1.0}, "constant")


def cumsum_mpo(fs) -> AxisMPO:
    """``y[o] = sum_{i <= o} x[i]``: the digits of ``i`` and ``o`` are compared coarse to fine in the states eq (0) and
    lt (1).  From eq, ``i < o`` goes to lt, ``i == o`` stays, ``i > o`` contributes nothing; from lt everything stays
    lt.  The chain starts in eq and accepts both states.  ``opnorm = n`` (the Frobenius norm of the triangle of ones
    is below it)."""
    f = _factors(fs)
    L = len(f)
    cores = []
    for k, v in enumerate(f):
        o, i = np.meshgrid(np.arange(v), np.arange(v), indexing="ij")
        t = np.zeros((2, v, v, 2))
        t[0, :, :, 0] = i == o
        t[0, :, :, 1] = i < o
        t[1, :, :, 1] = 1.0
        if k == L - 1:
            t = t.sum(axis=3, keepdims=True)
        if k == 0:
            t = t[:1]
        cores.append(t)
    return AxisMPO(cores, float(np.prod(f, dtype=np.int64)))


def flip_mpo(fs) -> AxisMPO:
    """``y[o] = x[n - 1 - o]``: every digit reversed, ``o = f_k - 1 - i``; bond 1, ``opnorm = 1``."""
    return AxisMPO([np.eye(v)[::-1].reshape(1, v, v, 1) for v in _factors(fs)], 1.0)


# ------------------------------------------------------------------------------------------------ application
def site_split(factor_arr, axis):
    """Per site (pre, f, post): the site's physical index is ``(p * f + digit) * post + q`` with ``p < pre`` the
    raveled digits of the earlier axes and ``q < post`` those of the later ones."""
    fa = np.asarray(factor_arr, dtype=np.int64)
    return [(int(np.prod(row[:axis], dtype=np.int64)), int(row[axis]), int(np.prod(row[axis + 1:], dtype=np.int64)))
            for row in fa]


def check_plan(mpo, factor_arr, axis, dims=None) -> None:
    """ValueError unless the operator's digits are those of ``axis`` in ``factor_arr`` (and ``dims`` its site dims)."""
    fa = np.asarray(factor_arr, dtype=np.int64)
    if fa.ndim != 2 or not 0 <= axis < fa.shape[1]:
        raise ValueError("factor_arr must be (L, ndim) and axis one of its columns")
    if mpo.factors != [int(v) for v in fa[:, axis]]:
        raise ValueError(f"the operator's digits {mpo.factors} are not those of axis {axis}: {fa[:, axis].tolist()}")
    if dims is not None and [int(d) for d in dims] != [int(v) for v in np.prod(fa, axis=1)]:
        raise ValueError("the chain's site dims are not those of factor_arr")


def emulate(cores, mpo, factor_arr, axis):
    """fp64 NumPy application of the operator to a list of ``(chi, d, chi')`` cores: the wide chain the device computes
    (module docstring), bonds ``D_k chi_k`` carry-major on both sides."""
    check_plan(mpo, factor_arr, axis, [np.shape(c)[1] for c in cores])
    out = []
    for x, m, (pre, f, post) in zip(cores, mpo.cores, site_split(factor_arr, axis)):
        x = np.asarray(x, dtype=np.float64)
        chi, d, chi2 = x.shape
        z = np.einsum("coid,apiqb->capoqdb", m, x.reshape(chi, pre, f, post, chi2))
        out.append(z.reshape(m.shape[0] * chi, d, m.shape[3] * chi2))
    return out
