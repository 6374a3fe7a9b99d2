"""Range and boolean metadata filters: Chroma's ``where`` grammar (``$eq $ne $gt $gte $lt $lte $in $nin $and $or``) over chunk metadata.

Three layers, each held to the one before it by the tests:

* ``matches(metadata, where)`` -- the specification: one chunk, plain Python.
* ``build_column`` / ``compile_where`` / ``WhereProgram.evaluate_numpy`` -- a typed int64 key column per field, and the filter as a
  postfix program over leaves that are key intervals, membership in a sorted run of keys, or "the field is missing".  Every ordering
  question (strings, floats, non-integral bounds on integers) is settled here, on the host, so an evaluator compares int64 keys only.
* ``DenseIndex.eval_where`` -- the same program on the device (``csrc/vf_where.h`` / ``vf_where.hip``), when it fits the limits below.

Semantics.  ``v = metadata.get(field)``; a missing field is ``None``: it passes ``$eq None``, an ``$in`` that lists ``None``, ``$ne x`` and
``$nin [...]`` when ``None`` is not among the values, and fails every ordering operator.  ``$ne`` is "not ``$eq``", ``$nin`` is "not ``$in``".
Several operators on a field, and several keys of a dict, are ANDed.  A scalar stands for ``{"$eq": scalar}``, a list / tuple / set /
frozenset for ``{"$in": [...]}``.  The present values of a field share one KIND -- ``bool`` (tested before ``int``), ``int`` (within int64),
``number`` (floats, or ints of magnitude <= 2**53 mixed with floats; no NaN; -0.0 is +0.0), ``str`` (ordered by code point) -- and a
comparison value must be of the field's kind (ints and floats both serve ``int`` and ``number`` fields).
"""
from __future__ import annotations

import bisect
import math

import numpy as np

COMPARE_OPS = ("$eq", "$ne", "$gt", "$gte", "$lt", "$lte", "$in", "$nin")
LOGICAL_OPS = ("$and", "$or")
_ORDERING = ("$gt", "$gte", "$lt", "$lte")

# the device evaluator's limits (csrc/vf_where.h holds the same figures): a program beyond them is evaluated by evaluate_numpy
MAX_LEAVES, MAX_OPS, MAX_DEPTH, MAX_COLUMNS, MAX_SET_VALUES = 64, 128, 32, 16, 65536
IN_AS_INTERVALS = 4            # an $in of up to this many values is ORed intervals, a longer one a set leaf
OP_AND, OP_OR, OP_NOT = 0x80, 0x81, 0x82   # an op below 0x80 pushes that leaf
_AND, _OR, _NOT = -1, -2, -3             # the same three in WhereProgram.code, where any int >= 0 pushes a leaf
_DEVICE_OP = {_AND: OP_AND, _OR: OP_OR, _NOT: OP_NOT}
LEAF_INTERVAL, LEAF_SET, LEAF_MISSING = 0, 1, 2
KEY_MIN, KEY_MAX = -(1 << 63), (1 << 63) - 1
_BIG = 1 << 70                 # stands for an infinite bound among Python ints

LEAF_DTYPE = np.dtype([("kind", np.int32), ("column", np.int32), ("lo", np.int64), ("hi", np.int64)])   # vf_where_leaf


# ---- values ------------------------------------------------------------------------------------------------------------------------
def kind_of(v):
    """'bool' / 'int' / 'float' / 'str', None for None, else the type's name (no filter can be built on it)."""
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)):
        return "bool"
    if isinstance(v, (int, np.integer)):
        return "int"
    if isinstance(v, (float, np.floating)):
        return "float"
    if isinstance(v, str):
        return "str"
    return type(v).__name__


def _class(kind):
    return "number" if kind in ("int", "float") else kind


def _scalar(v, what: str):
    k = kind_of(v)
    if k not in (None, "bool", "int", "float", "str"):
        raise ValueError(f"where: {what} must be a bool, int, float, str or None, got {k}")
    if k == "float" and math.isnan(v):
        raise ValueError(f"where: {what} is NaN")
    return v


# ---- the grammar -------------------------------------------------------------------------------------------------------------------
def has_operators(where) -> bool:
    """A ``$`` key anywhere in ``where``: the filter speaks the operator grammar (else it is the plain field -> value(s) form)."""
    if isinstance(where, dict):
        return any((isinstance(k, str) and k.startswith("$")) or has_operators(v) for k, v in where.items())
    if isinstance(where, (list, tuple)):
        return any(has_operators(x) for x in where if isinstance(x, (dict, list, tuple)))
    return False


def _member(field, op, values):
    """The node of an $in / $nin: its fifth entry is the values as a set of (kind class, value), so that asking costs one lookup --
    equal numbers hash alike whatever their type, and True is kept apart from 1 by its class."""
    return ("cmp", field, op, values, frozenset((_class(kind_of(e)), e) for e in values))


def _listed(v, node) -> bool:
    try:
        return (_class(kind_of(v)), v) in node[4]
    except TypeError:      # an unhashable metadata value (a list): it equals no filter value
        return False


def parse(where):
    """``where`` as a tree: ("and" | "or", [nodes]) and ("cmp", field, op, value) -- value a list for $in / $nin (``_member``).  Raises ValueError
    (naming the offender) for an unknown ``$name``, an empty ``$and`` / ``$or`` / ``$in`` list, an empty operator dict, a ``$`` key where a
    field is expected."""
    if not isinstance(where, dict):
        raise ValueError(f"where: a filter is a dict, got {type(where).__name__}")
    terms = []
    for key, val in where.items():
        if key in LOGICAL_OPS:
            if not isinstance(val, (list, tuple)) or len(val) == 0:
                raise ValueError(f"where: {key} takes a non-empty list of filters (empty {key} list)" if isinstance(val, (list, tuple))
                                 else f"where: {key} takes a non-empty list of filters, got {type(val).__name__}")
            terms.append(("and" if key == "$and" else "or", [parse(w) for w in val]))
            continue
        if isinstance(key, str) and key.startswith("$"):
            if key in COMPARE_OPS:
                raise ValueError(f"where: operator {key!r} where a field is expected")
            raise ValueError(f"where: unknown operator {key!r}")
        field = key
        if isinstance(val, dict):
            if not val:
                raise ValueError(f"where: empty operator dict on field {field!r}")
            for op, x in val.items():
                if op not in COMPARE_OPS:
                    raise ValueError(f"where: unknown operator {op!r} on field {field!r}")
                if op in ("$in", "$nin"):
                    if not isinstance(x, (list, tuple, set, frozenset)):
                        raise ValueError(f"where: {op} on field {field!r} takes a list of values, got {type(x).__name__}")
                    if len(x) == 0:
                        raise ValueError(f"where: empty {op} list on field {field!r}")
                    terms.append(_member(field, op, [_scalar(e, f"a value of {op} on field {field!r}") for e in x]))
                else:
                    x = _scalar(x, f"the value of {op} on field {field!r}")
                    if x is None and op in _ORDERING:
                        raise ValueError(f"where: {op} on field {field!r} cannot compare with None")
                    terms.append(("cmp", field, op, x))
        elif isinstance(val, (list, tuple, set, frozenset)):
            if len(val) == 0:
                raise ValueError(f"where: empty $in list on field {field!r}")
            terms.append(_member(field, "$in", [_scalar(e, f"a value listed for field {field!r}") for e in val]))
        else:
            terms.append(("cmp", field, "$eq", _scalar(val, f"the value of field {field!r}")))
    return ("and", terms)


def fields_of(where) -> list:
    """The fields ``where`` names, in order of first appearance."""
    out = []

    def walk(node):
        if node[0] == "cmp":
            if node[1] not in out:
                out.append(node[1])
        else:
            for c in node[1]:
                walk(c)
    walk(parse(where))
    return out


def _equal(v, x) -> bool:
    if v is None or x is None:
        return v is None and x is None
    kv, kx = _class(kind_of(v)), _class(kind_of(x))
    return kv == kx and kv in ("bool", "number", "str") and bool(v == x)


def _ordered(v, op, x) -> bool:
    if v is None:
        return False
    kv, kx = _class(kind_of(v)), _class(kind_of(x))
    if kv != kx or kv not in ("bool", "number", "str"):
        return False
    if kv == "number" and kind_of(v) == "float" and math.isnan(v):
        return False
    return bool(v > x if op == "$gt" else v >= x if op == "$gte" else v < x if op == "$lt" else v <= x)


def _eval(node, md) -> bool:
    if node[0] == "and":
        return all(_eval(c, md) for c in node[1])
    if node[0] == "or":
        return any(_eval(c, md) for c in node[1])
    field, op, x = node[1], node[2], node[3]
    v = md.get(field)
    if op == "$eq":
        return _equal(v, x)
    if op == "$ne":
        return not _equal(v, x)
    if op == "$in":
        return _listed(v, node)
    if op == "$nin":
        return not _listed(v, node)
    return _ordered(v, op, x)


def matches(metadata, where) -> bool:
    """Does one chunk's metadata pass ``where``?  Plain Python: the specification every other route is held to."""
    return _eval(parse(where), metadata)


def matcher(where):
    """``lambda metadata: matches(metadata, where)`` with ``where`` parsed once: for asking about many chunks."""
    tree = parse(where)
    return lambda metadata: _eval(tree, metadata)


# ---- columns -----------------------------------------------------------------------------------------------------------------------
def float_key(x) -> np.ndarray:
    """float64 -> int64 whose signed order is the floats' order; -0.0 gets the key of +0.0."""
    b = (np.asarray(x, dtype=np.float64) + 0.0).view(np.int64)
    return b ^ ((b >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))


class WhereColumn:
    """One field of every chunk as int64 keys: ``kind`` ('bool', 'int', 'number', 'str', or None when no chunk has the field), ``keys``
    [n], ``valid`` (bool [n]; None when every row has the field) and, for 'str', ``values``: the sorted distinct strings whose ranks the
    keys are.  ``_device`` keeps the device copies ``DenseIndex.eval_where`` uploads on first use."""

    def __init__(self, kind, keys, valid, values=None, field=""):
        self.kind, self.keys, self.valid, self.values, self.field = kind, keys, valid, values, field
        self.n = int(keys.shape[0])
        self._device = {}

    def valid_words(self) -> np.ndarray:
        """``valid`` as the evaluator reads it: uint32 words, bit r & 31 of word r >> 5, 2 * ceil(n / 64) of them, zero past n."""
        words = np.zeros(2 * ((self.n + 63) // 64), dtype=np.uint32)
        if self.n:
            packed = np.packbits(self.valid, bitorder="little")
            words.view(np.uint8)[:packed.size] = packed
        return words


def build_column(values, field: str = "") -> WhereColumn:
    """The column of one field: ``values[r]`` is ``metadata[r].get(field)``.  ValueError (naming the field and the kinds found) when the
    present values do not share one kind, an int lies outside int64 (or outside +-2**53 beside floats), or a float is NaN."""
    n = len(values)
    kinds = {}
    for v in values:
        k = kind_of(v)
        if k is not None:
            kinds[k] = kinds.get(k, 0) + 1
    names = set(kinds)
    if not names:
        return WhereColumn(None, np.zeros(n, np.int64), np.zeros(n, np.bool_), field=field)
    if names == {"bool"}:
        kind = "bool"
    elif names == {"int"}:
        kind = "int"
    elif names <= {"int", "float"}:
        kind = "number"
    elif names == {"str"}:
        kind = "str"
    else:
        raise ValueError(f"where: field {field!r} holds values of kinds {sorted(names)}: a filtered field's values must all be bool, "
                         "all int, all numbers (int and float) or all str")
    present = sum(kinds.values())
    valid = None if present == n else np.fromiter((v is not None for v in values), np.bool_, n)
    keys = np.zeros(n, np.int64)
    rows = np.arange(n) if valid is None else np.flatnonzero(valid)
    have = values if valid is None else [v for v in values if v is not None]
    distinct = None
    if kind == "bool":
        keys[rows] = np.fromiter((1 if v else 0 for v in have), np.int64, present)
    elif kind == "int":
        for v in have:
            if not KEY_MIN <= int(v) <= KEY_MAX:
                raise ValueError(f"where: field {field!r} holds the int {v}, outside int64")
        keys[rows] = np.fromiter((int(v) for v in have), np.int64, present)
    elif kind == "number":
        for v in have:
            if kind_of(v) == "int" and abs(int(v)) > (1 << 53):
                raise ValueError(f"where: field {field!r} mixes floats with the int {v}, of magnitude above 2**53")
        f = np.fromiter((float(v) for v in have), np.float64, present)
        if np.isnan(f).any():
            raise ValueError(f"where: field {field!r} holds NaN")
        keys[rows] = float_key(f)
    else:
        distinct = sorted(set(have))
        rank = {s: i for i, s in enumerate(distinct)}
        keys[rows] = np.fromiter((rank[v] for v in have), np.int64, present)
    return WhereColumn(kind, keys, valid, distinct, field)


# ---- compiling ---------------------------------------------------------------------------------------------------------------------
def _int_bounds(x):
    """(floor, ceil) of a comparison value as Python ints; an infinity becomes +-2**70."""
    if kind_of(x) == "int":
        return int(x), int(x)
    if math.isinf(x):
        return (_BIG, _BIG) if x > 0 else (-_BIG, -_BIG)
    return math.floor(x), math.ceil(x)


def _float_bounds(x):
    """(largest float64 <= x, smallest float64 >= x) of a comparison value (Python compares an int and a float exactly)."""
    if kind_of(x) == "float":
        f = float(x) + 0.0
        return f, f
    try:
        f = float(int(x))
    except OverflowError:
        return (float(np.finfo(np.float64).max), math.inf) if x > 0 else (-math.inf, -float(np.finfo(np.float64).max))
    if f == x:
        return f, f
    return (float(np.nextafter(f, -math.inf)), f) if f > x else (f, float(np.nextafter(f, math.inf)))


def _check_value(col: WhereColumn, op: str, x) -> None:
    if x is None or col.kind is None:
        return
    k = kind_of(x)
    ok = (k == "bool") if col.kind == "bool" else (k in ("int", "float")) if col.kind in ("int", "number") else (k == "str")
    if not ok:
        raise ValueError(f"where: field {col.field!r} is of kind {col.kind}, the {op} value {x!r} is of kind {k}")


def _interval(col: WhereColumn, op: str, x):
    """The inclusive key interval (lo, hi), as unbounded Python ints, of the rows with ``field op x`` (x not None)."""
    lo, hi = -_BIG, _BIG
    if col.kind is None:
        return 1, 0
    if col.kind in ("bool", "int"):
        fl, ce = (int(x), int(x)) if col.kind == "bool" else _int_bounds(x)
        if op == "$eq":
            return (fl, fl) if fl == ce else (1, 0)
        if op == "$gt":
            lo = fl + 1
        elif op == "$gte":
            lo = ce
        elif op == "$lt":
            hi = ce - 1
        else:
            hi = fl
        return lo, hi
    if col.kind == "number":
        below, above = _float_bounds(x)
        kb, ka = int(float_key(below)), int(float_key(above))
        if op == "$eq":
            return (kb, kb) if below == above else (1, 0)
        if op == "$gt":
            lo = kb + 1
        elif op == "$gte":
            lo = ka
        elif op == "$lt":
            hi = ka - 1
        else:
            hi = kb
        return lo, hi
    left, right = bisect.bisect_left(col.values, x), bisect.bisect_right(col.values, x)
    if op == "$eq":
        return (left, left) if right > left else (1, 0)
    if op == "$gt":
        lo = right
    elif op == "$gte":
        lo = left
    elif op == "$lt":
        hi = left - 1
    else:
        hi = right - 1
    return lo, hi


def _clamp(lo, hi):
    lo, hi = max(lo, KEY_MIN), min(hi, KEY_MAX)
    return (1, 0) if lo > hi else (lo, hi)


class WhereProgram:
    """A compiled filter: ``fields`` (the columns it names, in order), ``leaves`` (LEAF_DTYPE), ``code`` (postfix: an int >= 0 pushes
    that leaf; -1 and, -2 or, -3 not), ``set_values`` (int64: the set leaves' strictly ascending runs, back to back) and ``depth``, the
    deepest the evaluation stack gets.  ``ops`` is ``code`` as the device reads it (uint8: a value below 0x80 pushes that leaf)."""

    def __init__(self, fields, leaves, code, set_values, depth, n):
        self.fields, self.leaves, self.code, self.set_values, self.depth, self.n = tuple(fields), leaves, list(code), set_values, int(depth), int(n)

    @property
    def ops(self) -> np.ndarray:
        if len(self.leaves) > MAX_LEAVES:
            raise ValueError("where: a program of more than 64 leaves has no device encoding")
        return np.asarray([c if c >= 0 else _DEVICE_OP[c] for c in self.code], np.uint8)

    @property
    def fits_device(self) -> bool:
        return (1 <= len(self.fields) <= MAX_COLUMNS and 1 <= len(self.leaves) <= MAX_LEAVES and 1 <= len(self.code) <= MAX_OPS
                and self.depth <= MAX_DEPTH and len(self.set_values) <= MAX_SET_VALUES)

    def evaluate_numpy(self, columns, n: int = None) -> np.ndarray:
        """The bool mask [n] of the passing rows: the program run over whole columns (``columns``: field -> WhereColumn)."""
        cols = [columns[f] for f in self.fields]
        n = self.n if n is None else int(n)
        for c in cols:
            if c.n != n:
                raise ValueError(f"where: the column of field {c.field!r} has {c.n} rows, the program was compiled for {n}")
        stack = []
        for op in self.code:
            if op >= 0:
                kind, ci, lo, hi = (int(v) for v in self.leaves[op].tolist())
                if kind == LEAF_INTERVAL:
                    if lo > hi:
                        m = np.zeros(n, np.bool_)
                    else:
                        c = cols[ci]
                        m = (c.keys >= lo) & (c.keys <= hi)
                        if c.valid is not None:
                            m &= c.valid
                elif kind == LEAF_SET:
                    c = cols[ci]
                    m = np.isin(c.keys, self.set_values[lo:lo + hi])
                    if c.valid is not None:
                        m &= c.valid
                else:
                    c = cols[ci]
                    m = np.zeros(n, np.bool_) if c.valid is None else ~c.valid
                stack.append(m)
            elif op == _NOT:
                stack[-1] = ~stack[-1]
            else:
                b = stack.pop()
                stack[-1] = (stack[-1] & b) if op == _AND else (stack[-1] | b)
        assert len(stack) == 1
        return stack[0]


def compile_where(where, columns, n: int = None) -> WhereProgram:
    """``where`` over ``columns`` (field -> WhereColumn, at least the fields ``fields_of(where)`` names) as a WhereProgram.  ValueError
    for a comparison value that is not of its field's kind."""
    tree = parse(where)
    fields, leaves, leaf_at, sets = [], [], {}, []
    set_len = [0]

    def column_of(field):
        if field not in fields:
            fields.append(field)
        return fields.index(field), columns[field]

    def leaf(kind, ci, lo, hi):
        key = (kind, ci, lo, hi)
        if kind == LEAF_SET or key not in leaf_at:    # equal interval / missing leaves are shared
            leaf_at[key] = len(leaves)
            leaves.append(key)
        return ("leaf", leaf_at[key])

    def member(ci, col, op, xs):
        """field in xs"""
        for x in xs:
            _check_value(col, op, x)
        alts = [leaf(LEAF_MISSING, ci, 0, 0)] if any(x is None for x in xs) else []
        given = [x for x in xs if x is not None]
        keys = sorted({iv[0] for iv in (_clamp(*_interval(col, "$eq", x)) for x in given) if iv[0] <= iv[1]})
        if len(given) <= IN_AS_INTERVALS:
            alts += [leaf(LEAF_INTERVAL, ci, k, k) for k in keys]
        elif keys:
            alts.append(leaf(LEAF_SET, ci, set_len[0], len(keys)))
            sets.extend(keys)
            set_len[0] += len(keys)
        if not alts:
            return leaf(LEAF_INTERVAL, ci, 1, 0)
        return alts[0] if len(alts) == 1 else ("or", alts)

    def build(node):
        if node[0] in ("and", "or"):
            if node[0] == "and":      # the comparisons of one field that are intervals merge into one leaf
                return conj(node[1])
            kids = [build(c) for c in node[1]]
            return kids[0] if len(kids) == 1 else ("or", kids)
        return conj([node])

    def conj(nodes):
        out, spans = [], {}
        for node in nodes:
            if node[0] != "cmp":
                out.append(build(node))
                continue
            field, op, x = node[1], node[2], node[3]
            ci, col = column_of(field)
            if op in ("$in", "$nin"):
                t = member(ci, col, op, x)
                out.append(t if op == "$in" else ("not", t))
                continue
            _check_value(col, op, x)
            if op in ("$eq", "$ne") and x is None:
                t = leaf(LEAF_MISSING, ci, 0, 0)
                out.append(t if op == "$eq" else ("not", t))
            elif op == "$ne":
                out.append(("not", leaf(LEAF_INTERVAL, ci, *_clamp(*_interval(col, "$eq", x)))))
            else:
                lo, hi = _interval(col, op, x)
                if ci in spans:      # (the empty interval is (1, 0): max / min keep it empty)
                    spans[ci][1], spans[ci][2] = max(spans[ci][1], lo), min(spans[ci][2], hi)
                else:
                    spans[ci] = [len(out), lo, hi]
                    out.append(None)
        for ci, (at, lo, hi) in spans.items():
            out[at] = leaf(LEAF_INTERVAL, ci, *_clamp(lo, hi))
        if not out:                     # an empty dict passes everything: not (the empty leaf)
            return ("not", leaf(LEAF_INTERVAL, 0, 1, 0))
        return out[0] if len(out) == 1 else ("and", out)

    root = build(tree)
    ops = []
    depth = [0, 0]   # now, deepest

    def emit(node):
        if node[0] == "leaf":
            ops.append(node[1])
            depth[0] += 1
            depth[1] = max(depth[1], depth[0])
        elif node[0] == "not":
            emit(node[1])
            ops.append(_NOT)
        else:
            emit(node[1][0])
            for c in node[1][1:]:
                emit(c)
                ops.append(_AND if node[0] == "and" else _OR)
                depth[0] -= 1
    emit(root)
    if n is None:
        ns = {columns[f].n for f in fields}
        if len(ns) > 1:
            raise ValueError("where: the columns have different row counts")
        n = ns.pop() if ns else 0
    arr = np.zeros(len(leaves), LEAF_DTYPE)
    for i, (kind, ci, lo, hi) in enumerate(leaves):
        arr[i] = (kind, ci, lo, hi)
    return WhereProgram(fields, arr, ops, np.asarray(sets, np.int64), depth[1], n)


# ---- the passing rows as a set -------------------------------------------------------------------------------------------------------
class RowMask:
    """The passing rows as the ensemble's ``allow``: ``r in mask`` (False outside [0, n): the neighbour expansion asks about -1),
    ``len(mask)`` = rows passing, iteration in ascending order.  Wraps the bool array an evaluation produced; no Python set is built."""

    def __init__(self, mask: np.ndarray, count: int = None):
        self.mask = np.asarray(mask, dtype=np.bool_)
        self._count = int(np.count_nonzero(self.mask)) if count is None else int(count)

    @classmethod
    def from_words(cls, words: np.ndarray, n: int, count: int = None) -> "RowMask":
        """From the evaluator's bitmap: uint32 words, bit r & 31 of word r >> 5."""
        bits = np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")
        return cls(bits[:n].astype(np.bool_), count)

    def __contains__(self, r) -> bool:
        return 0 <= r < self.mask.shape[0] and bool(self.mask[r])

    def __len__(self) -> int:
        return self._count

    def __iter__(self):
        return iter(np.flatnonzero(self.mask).tolist())
