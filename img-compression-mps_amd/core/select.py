"""Voxels by value from the cores: how many lie in an interval, which ones, which are NaN, which k are the largest.

The host side of csrc/select.hip (``ndmps_select_*``), the one epilogue of the statistics family whose output is a list:
the chain is contracted as ``to_tensor`` contracts it and the last product -- the only one that touches N elements --
appends ``(flat C-order index, value)`` of every matching voxel to a list instead of storing the volume.
``NDMPS.count_between`` / ``find`` / ``find_nan`` / ``topk`` are thin methods over the functions below.

Count, then emit.  ``find`` first counts with the clipped moments pass (``valstat.moments``), refuses more than
``max_count`` matches, allocates exactly that many slots and runs the list pass with ``capacity = count``; the entry
returns the number of matches it saw, which must be the count.  The bounds are cast to the cores' element type here and
the predicate is evaluated on the computed voxel in that type, so ``count_between(lo, hi)``, ``len(find(lo, hi)[0])``
and the one bin of ``histogram(bins=[lo, hi])`` agree exactly.  The kernel hands out slots in order of arrival; the K
pairs are then sorted by their index on the device, and since flat indices are unique the same inputs give the same
bytes.

``topk`` brackets the k-th value with histogram passes (``valstat.bin_counts``, at most 4096 bins each, their edges
evenly spaced in the order-preserving key so that a pass divides the numbers inside the bracket by 4096) until the
half-line from the bracket's inner edge holds at most ``max_count`` voxels or the bracket is one number ``t``, then
calls ``find`` on that half-line, orders by (value, index) and takes k.  Where too many voxels tie at ``t`` it takes
the strictly better ones with one ``find`` and the first ``k - c`` ties in C order from ``find(t, t)``.  That logic,
``topk_select``, sees the volume only through a small backend (``moments``, ``bin_counts``, ``find``), so
tests/test_select_cases_host.py runs it on a NumPy stand-in.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from . import valstat as _vs

INSIDE, OUTSIDE, NAN = 0, 1, 2
MAX_COUNT = 1 << 20

_torch = _vs._torch


# ------------------------------------------------------------------------------------------------ arguments
def check_max_count(max_count):
    if isinstance(max_count, bool) or not isinstance(max_count, (int, np.integer)):
        raise TypeError("max_count must be an integer")
    if max_count < 0:
        raise ValueError(f"max_count must not be negative, got {int(max_count)}")
    return int(max_count)


def check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError("k must be an integer")
    if k < 1:
        raise ValueError(f"k must be at least 1, got {int(k)}")
    return int(k)


def bounds(lo, hi, np_type):
    """``(lo, hi)`` in the element type ``np_type``; None is unbounded.  ValueError for a NaN bound and ``lo > hi``."""
    with np.errstate(over="ignore"):
        lo = np_type(-np.inf) if lo is None else np_type(lo)
        hi = np_type(np.inf) if hi is None else np_type(hi)
    if np.isnan(lo) or np.isnan(hi):
        raise ValueError("a bound of the interval is NaN: find_nan lists the NaN voxels")
    if lo > hi:
        raise ValueError(f"the interval is empty: lo = {lo} > hi = {hi}")
    return lo, hi


def check_find(chain, lo, hi, max_count):
    """The refusals of ``find`` / ``find_nan`` that need no device; returns ``(lo, hi)`` in the element type and
    ``max_count``."""
    np_type, _ = _vs._element(chain)
    max_count = check_max_count(max_count)
    return bounds(lo, hi, np_type) + (max_count,)


def check_topk(chain, k, max_count):
    """The refusals of ``topk`` that need no device; returns ``(k, max_count, element type)``."""
    np_type, _ = _vs._element(chain)
    return check_k(k), check_max_count(max_count), np_type


def too_many(count, max_count, what):
    return ValueError(f"{what}: {count} voxels match, more than max_count = {max_count}; narrow the interval or raise max_count")


# ------------------------------------------------------------------------------------------------ the device calls
def _counts(chain, lo, hi):
    """(inside, outside and not NaN, NaN) of the interval, bounds in the element type: the clipped moments pass."""
    m = _vs.moments(chain, clip=(float(lo), float(hi)))
    return m["taken"], m["count"] - m["n_nan"] - m["taken"], m["n_nan"]


def count_between(chain, lo=None, hi=None, invert=False):
    """The number of non-NaN voxels with ``lo <= v <= hi`` (None: unbounded), or with ``invert`` outside it: an int."""
    np_type, _ = _vs._element(chain)
    lo, hi = bounds(lo, hi, np_type)
    inside, outside, _ = _counts(chain, lo, hi)
    return int(outside if invert else inside)


def _empty(chain):
    torch = _torch()
    return (torch.empty(0, dtype=torch.int64, device=chain.device), torch.empty(0, dtype=chain.dtype, device=chain.device))


def emit(chain, plan, mode, lo, hi, count):
    """The ``count`` matches of ``mode`` (INSIDE, OUTSIDE, NAN) as device tensors ``(index int64 ascending, values)``:
    the list pass with exactly ``count`` slots, then the sort of the pairs by index.  ``count`` is what the moments
    pass counted; another total from the list pass is an internal error."""
    torch = _torch()
    if count == 0:
        return _empty(chain)
    device = chain.device
    n_cols = _vs._split_columns(chain)
    with torch.cuda.device(device):
        row_off, col_off, col_perm = plan.split_tables(n_cols, device)
        call = _vs._Call(chain)
        index = torch.empty(count, dtype=torch.int64, device=device)
        values = torch.empty(count, dtype=chain.dtype, device=device)
        total = C.c_int64()
        _lib.check(call.entry("select")(*call.head(), int(mode), float(lo), float(hi), row_off.data_ptr(), col_off.data_ptr(),
                                        col_perm.data_ptr(), n_cols, count, index.data_ptr(), values.data_ptr(),
                                        C.byref(total), *call.tail()))
        if int(total.value) != count:
            raise RuntimeError(f"internal: the list pass saw {int(total.value)} matches, the moments pass counted {count}")
        index, order = torch.sort(index)
        return index, values[order]


def find_device(chain, plan, lo=None, hi=None, invert=False, max_count=MAX_COUNT, what="find"):
    """``find`` as device tensors ``(index ascending, values)``."""
    lo, hi, max_count = check_find(chain, lo, hi, max_count)
    inside, outside, _ = _counts(chain, lo, hi)
    count = outside if invert else inside
    if count > max_count:
        raise too_many(count, max_count, what)
    return emit(chain, plan, OUTSIDE if invert else INSIDE, lo, hi, count)


def find_nan_device(chain, plan, max_count=MAX_COUNT):
    max_count = check_find(chain, None, None, max_count)[2]
    n_nan = _vs.moments(chain)["n_nan"]
    if n_nan > max_count:
        raise too_many(n_nan, max_count, "find_nan")
    return emit(chain, plan, NAN, 0.0, 0.0, n_nan)[0]


# ------------------------------------------------------------------------------------------------ results
def _index_result(index, shape, coords, as_torch):
    """Flat indices, or with ``coords`` their ``np.unravel_index`` as a (K, ndim) int64 array."""
    torch = _torch()
    if not coords:
        return index if as_torch else index.cpu().numpy()
    if not as_torch:
        flat = index.cpu().numpy()
        return np.stack(np.unravel_index(flat, shape), axis=1).astype(np.int64).reshape(flat.size, len(shape))
    cols, rest = [], index
    for n in reversed(shape):
        cols.append(rest % n)
        rest = torch.div(rest, n, rounding_mode="floor")
    return torch.stack(cols[::-1], dim=1)


def _pair_result(index, values, shape, coords, as_torch):
    return _index_result(index, shape, coords, as_torch), (values if as_torch else values.cpu().numpy())


def find(chain, plan, lo=None, hi=None, invert=False, max_count=MAX_COUNT, coords=False, as_torch=False):
    """``(index, values)`` of the non-NaN voxels with ``lo <= v <= hi`` (``invert``: outside): ``np.flatnonzero`` of the
    predicate on the volume, ascending int64, and the values there in the element type.  ValueError naming the count for
    more than ``max_count`` matches."""
    index, values = find_device(chain, plan, lo, hi, invert, max_count)
    return _pair_result(index, values, plan.shape, coords, as_torch)


def find_nan(chain, plan, max_count=MAX_COUNT, coords=False, as_torch=False):
    """The flat indices (``coords``: coordinates) of the NaN voxels, ascending."""
    return _index_result(find_nan_device(chain, plan, max_count), plan.shape, coords, as_torch)


# ------------------------------------------------------------------------------------------------ top k
def _keys(x):
    """The order-preserving unsigned keys of an array of the element type (ext_key of csrc/valstat_device.h): the bits
    with the sign bit set for v >= 0 and all bits flipped for v < 0, -0 made +0 first."""
    x = np.atleast_1d(x) + x.dtype.type(0)
    utype = np.uint32 if x.dtype == np.float32 else np.uint64
    b = x.view(utype)
    sign = utype(1) << utype(8 * x.dtype.itemsize - 1)
    return np.where(b & sign, ~b, b | sign)


def _values(keys, np_type):
    utype = np.uint32 if np_type == np.float32 else np.uint64
    k = np.asarray(keys, dtype=utype)
    sign = utype(1) << utype(8 * k.dtype.itemsize - 1)
    return np.where(k & sign, k ^ sign, ~k).view(np_type)


def bracket_edges(lo, hi, np_type, bins=_vs.MAX_BINS):
    """Strictly ascending edges in the element type from ``lo`` to ``hi`` (``lo < hi``), at most ``bins`` bins, evenly
    spaced in the order-preserving key: a pass divides the numbers of the element type inside the bracket by ``bins``
    whatever their magnitudes, so three passes (fp32) or six (fp64) reach a single number from any bracket,
    infinite ends included."""
    a, b = (int(k) for k in _keys(np.array([lo, hi], dtype=np_type)))
    n = min(int(bins), b - a)
    keys = [a + (b - a) * i // n for i in range(n + 1)]
    return np.unique(_values(keys, np_type))


def topk_select(be, k, largest, max_count, np_type):
    """``(index, values)`` of the ``k`` largest (smallest) non-NaN voxels, by value and among equal values by ascending
    index, from a backend ``be`` with

      ``moments()``                 dict with count, n_nan, min, max
      ``count(lo, hi)``             voxels with lo <= v <= hi
      ``bin_counts(edges)``         (counts, n_below, n_above, n_nan), numpy.histogram's bins, the last one closed
      ``find(lo, hi, count)``       (index ascending, values) of the ``count`` voxels with lo <= v <= hi
      ``best(index, values, k, largest)``   the first k pairs by (value, index)
      ``concat(pairs)``             one pair from several

    The bracket [lo, hi] always holds the k-th value: fewer than k voxels lie strictly beyond its outer edge and at
    least k (``reach``, known from the counts) at or beyond its inner edge."""
    inf = np_type(np.inf)
    m = be.moments()
    n = m["count"] - m["n_nan"]
    k = min(k, n)
    if k == 0:
        return be.find(inf, -inf, 0)  # nothing: the backend's empty pair
    if k > max_count:
        raise ValueError(f"topk: k = {k} voxels are more than max_count = {max_count}")
    lo, hi = np_type(m["min"]), np_type(m["max"])
    reach, beyond = n, 0  # voxels at or beyond the inner edge; voxels strictly beyond the outer edge
    up = lambda x: np.nextafter(x, inf)       # noqa: E731
    down = lambda x: np.nextafter(x, -inf)    # noqa: E731
    while reach > max_count and lo < hi:
        edges = bracket_edges(lo, hi, np_type)
        if edges.size == 2:  # no edge fell inside: split off the inner end's neighbour by a count
            if largest:
                mid = up(lo)
                c = beyond + be.count(mid, hi)
                if c >= k:
                    lo, reach = mid, c
                else:
                    hi, beyond = lo, c
            else:
                mid = down(hi)
                c = beyond + be.count(lo, mid)
                if c >= k:
                    hi, reach = mid, c
                else:
                    lo, beyond = hi, c
            continue
        counts, below, above, _ = be.bin_counts(edges)
        last = counts.size - 1
        if largest:
            at_or_above = above + np.cumsum(counts[::-1])[::-1]  # voxels >= edges[b]
            b = int(np.flatnonzero(at_or_above >= k)[-1])
            reach = int(at_or_above[b])
            beyond = int(at_or_above[b + 1]) if b < last else int(above)
        else:
            up_to = below + np.cumsum(counts)  # voxels < edges[b + 1], the last bin: <= edges[b + 1]
            b = int(np.flatnonzero(up_to >= k)[0])
            reach = int(up_to[b])
            beyond = int(up_to[b - 1]) if b > 0 else int(below)
        lo, hi = edges[b], (edges[b + 1] if b == last else down(edges[b + 1]))  # the bin without its right edge
    if reach <= max_count:
        index, values = be.find(lo, inf, reach) if largest else be.find(-inf, hi, reach)
        return be.best(index, values, k, largest)
    # lo == hi == t and more than max_count voxels at or beyond it: the strictly better ones, then the first ties
    t = lo
    ties = reach - beyond
    if ties > max_count:
        raise ValueError(f"topk: {ties} voxels tie at the k-th value {t}, more than max_count = {max_count}")
    parts = []
    if beyond:
        index, values = be.find(up(t), inf, beyond) if largest else be.find(-inf, down(t), beyond)
        parts.append(be.best(index, values, beyond, largest))
    index, values = be.find(t, t, ties)
    parts.append((index[:k - beyond], values[:k - beyond]))
    return be.concat(parts)


class _DeviceBackend:
    """``topk_select``'s view of a chain: the passes of core/valstat.py and ``emit``, pairs as device tensors."""

    def __init__(self, chain, plan):
        self.chain, self.plan = chain, plan

    def moments(self):
        return _vs.moments(self.chain)

    def count(self, lo, hi):
        return _counts(self.chain, lo, hi)[0]

    def bin_counts(self, edges):
        return _vs.bin_counts(self.chain, np.ascontiguousarray(edges))

    def find(self, lo, hi, count):
        return emit(self.chain, self.plan, INSIDE, lo, hi, count)

    def best(self, index, values, k, largest):
        # a stable sort of the index-ascending pairs: equal values keep their ascending indices (-0.0 equals 0.0)
        _, order = _torch().sort(values, descending=bool(largest), stable=True)
        order = order[:k]
        return index[order], values[order]

    def concat(self, pairs):
        torch = _torch()
        return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])


def topk(chain, plan, k, largest=True, max_count=MAX_COUNT, coords=False, as_torch=False):
    """``(index, values)`` of the ``k`` largest (``largest=False``: smallest) non-NaN voxels, ordered by value and among
    equal values by ascending flat index (``np.lexsort((flat_index, -v))[:k]``); all of them where fewer than ``k`` are
    not NaN.  ValueError where ``k``, or the voxels that tie at the k-th value, exceed ``max_count``."""
    k, max_count, np_type = check_topk(chain, k, max_count)
    index, values = topk_select(_DeviceBackend(chain, plan), k, bool(largest), max_count, np_type)
    return _pair_result(index, values, plan.shape, coords, as_torch)
