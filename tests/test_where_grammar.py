"""The operator grammar of ``where`` (veritasfi_amd/where.py), on the CPU.

``matches`` -- the specification -- is held to HAND-WRITTEN rows on twelve chunks: every operator on each kind, missing fields under each
operator, None in $in / $nin, nesting three deep.  Every refusal carries its message.  The key maps keep order.  Then the compiled
program, run by ``evaluate_numpy``, equals ``matches`` on an enumerated family of filters over 300 seeded chunks (tests/where_cases.py)."""
import numpy as np
import pytest

import where_cases
from veritasfi_amd import where as W

INF = float("inf")
CHUNKS = [
    {"year": 2019, "company": "alpha", "score": 0.5, "public": True},        # 0
    {"year": 2020, "company": "beta", "score": 1.5, "public": False},        # 1
    {"year": 2021, "company": "alpha", "score": -2.0, "public": True},       # 2
    {"year": 2022, "company": "gamma", "score": 3, "public": False},         # 3   (an int among floats: kind number)
    {"year": 2023, "company": "beta", "score": 0.0, "public": True},         # 4
    {"company": "alpha", "score": -0.0},                                      # 5   no year, no public
    {"year": 2021, "score": 2.5, "public": False},                            # 6   no company
    {"year": 2024, "company": "Beta", "public": True},                        # 7   no score; "Beta" < "alpha" by code point
    {"year": 2020, "company": "délta", "score": 1e300, "public": False},      # 8
    {"year": 2022, "company": "alpha", "score": -1e-300},                     # 9   no public
    {"year": -5, "company": "", "score": INF, "public": True},                # 10
    {},                                                                       # 11
]
ALL = list(range(12))

EXPECTED = [
    # int
    ({"year": {"$eq": 2021}}, [2, 6]),
    ({"year": {"$ne": 2021}}, [0, 1, 3, 4, 5, 7, 8, 9, 10, 11]),
    ({"year": {"$gt": 2021}}, [3, 4, 7, 9]),
    ({"year": {"$gte": 2021}}, [2, 3, 4, 6, 7, 9]),
    ({"year": {"$lt": 2020}}, [0, 10]),
    ({"year": {"$lte": 2020}}, [0, 1, 8, 10]),
    ({"year": {"$in": [2019, 2024, 1999]}}, [0, 7]),
    ({"year": {"$nin": [2019, 2024, 1999]}}, [1, 2, 3, 4, 5, 6, 8, 9, 10, 11]),
    ({"year": {"$gt": 2020.5}}, [2, 3, 4, 6, 7, 9]),
    ({"year": {"$eq": 2020.5}}, []),
    ({"year": {"$eq": 2020.0}}, [1, 8]),
    ({"year": {"$lte": 2020.5}}, [0, 1, 8, 10]),
    ({"year": {"$gte": 2021, "$lt": 2023}}, [2, 3, 6, 9]),
    ({"year": {"$gt": 2022, "$lt": 2021}}, []),
    ({"year": {"$eq": None}}, [5, 11]),
    ({"year": {"$ne": None}}, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]),
    ({"year": {"$in": [None, 2023]}}, [4, 5, 11]),
    ({"year": {"$nin": [None, 2023]}}, [0, 1, 2, 3, 6, 7, 8, 9, 10]),
    ({"year": [2019, None], "company": {"$ne": "zzz"}}, [0, 5, 11]),
    ({"year": {"$lt": INF}}, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]),
    # str, by code point: "" < "Beta" < "alpha" < "beta" < "délta" < "gamma"
    ({"company": {"$eq": "alpha"}}, [0, 2, 5, 9]),
    ({"company": {"$ne": "alpha"}}, [1, 3, 4, 6, 7, 8, 10, 11]),
    ({"company": {"$gt": "alpha"}}, [1, 3, 4, 8]),
    ({"company": {"$gte": "alpha"}}, [0, 1, 2, 3, 4, 5, 8, 9]),
    ({"company": {"$lt": "alpha"}}, [7, 10]),
    ({"company": {"$lte": "Beta"}}, [7, 10]),
    ({"company": {"$gt": "b", "$lt": "e"}}, [1, 4, 8]),
    ({"company": {"$in": ["beta", "Beta", "nobody"]}}, [1, 4, 7]),
    ({"company": {"$nin": ["beta", "Beta", "nobody"]}}, [0, 2, 3, 5, 6, 8, 9, 10, 11]),
    ({"company": {"$gt": "zz"}}, []),
    ({"company": {"$gte": ""}}, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10]),
    ({"company": {"$eq": None}}, [6, 11]),
    # number: 0, 0.0 and -0.0 are one value
    ({"score": {"$eq": 0}}, [4, 5]),
    ({"score": {"$eq": -0.0}}, [4, 5]),
    ({"score": {"$gt": 0}}, [0, 1, 3, 6, 8, 10]),
    ({"score": {"$gte": 0.0}}, [0, 1, 3, 4, 5, 6, 8, 10]),
    ({"score": {"$lt": 0}}, [2, 9]),
    ({"score": {"$lte": -0.0}}, [2, 4, 5, 9]),
    ({"score": {"$ne": 3}}, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]),
    ({"score": {"$eq": 3.0}}, [3]),
    ({"score": {"$in": [0.5, 3, INF, 7]}}, [0, 3, 10]),
    ({"score": {"$nin": [0.5, 3, INF, 7]}}, [1, 2, 4, 5, 6, 7, 8, 9, 11]),
    ({"score": {"$gt": 2.5, "$lte": 1e300}}, [3, 8]),
    ({"score": {"$lt": INF}}, [0, 1, 2, 3, 4, 5, 6, 8, 9]),
    ({"score": {"$gte": -INF}}, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]),
    # bool
    ({"public": {"$eq": True}}, [0, 2, 4, 7, 10]),
    ({"public": {"$ne": True}}, [1, 3, 5, 6, 8, 9, 11]),
    ({"public": {"$gt": False}}, [0, 2, 4, 7, 10]),
    ({"public": {"$gte": False}}, [0, 1, 2, 3, 4, 6, 7, 8, 10]),
    ({"public": {"$lt": True}}, [1, 3, 6, 8]),
    ({"public": {"$lte": True}}, [0, 1, 2, 3, 4, 6, 7, 8, 10]),
    ({"public": {"$in": [False]}}, [1, 3, 6, 8]),
    ({"public": {"$nin": [False]}}, [0, 2, 4, 5, 7, 9, 10, 11]),
    ({"public": True, "year": {"$gte": 2021}}, [2, 4, 7]),
    # a field no chunk has
    ({"absent": {"$eq": None}}, ALL),
    ({"absent": {"$ne": 1}}, ALL),
    ({"absent": {"$eq": 1}}, []),
    ({"absent": {"$gt": 0}}, []),
    ({"absent": {"$lte": "z"}}, []),
    ({"absent": {"$in": ["x", None]}}, ALL),
    ({"absent": {"$nin": ["x"]}}, ALL),
    ({"absent": {"$nin": [None]}}, []),
    # nesting, three deep
    ({"$or": [{"$and": [{"company": "alpha"}, {"$or": [{"year": {"$lt": 2020}}, {"score": {"$lt": 0}}]}]},
              {"public": {"$eq": None}, "year": {"$eq": None}}]}, [0, 2, 5, 9, 11]),
    ({"$and": [{"$or": [{"year": 2020}, {"year": 2022}]},
               {"$or": [{"public": False}, {"$and": [{"score": {"$lt": 0}}, {"company": {"$ne": "beta"}}]}]}]}, [1, 3, 8, 9]),
    ({"$and": [{}]}, ALL),
]


def _columns(mds, where):
    return {f: W.build_column([md.get(f) for md in mds], f) for f in W.fields_of(where)}


@pytest.mark.parametrize("case", range(len(EXPECTED)))
def test_matches_by_hand(case):
    where, want = EXPECTED[case]
    assert [r for r, md in enumerate(CHUNKS) if W.matches(md, where)] == want, where
    program = W.compile_where(where, _columns(CHUNKS, where), n=len(CHUNKS))
    assert np.flatnonzero(program.evaluate_numpy(_columns(CHUNKS, where), len(CHUNKS))).tolist() == want, where


@pytest.mark.parametrize("where, message", [
    ({"$foo": [{"year": 1}]}, "unknown operator '$foo'"),
    ({"$and": []}, "empty $and list"),
    ({"$or": []}, "empty $or list"),
    ({"$or": [{"year": 1}, {"$and": []}]}, "empty $and list"),
    ({"year": {"$in": []}}, "empty $in list on field 'year'"),
    ({"year": {"$nin": []}}, "empty $nin list on field 'year'"),
    ({"year": [], "$and": [{"year": 1}]}, "empty $in list on field 'year'"),
    ({"year": {}, "$and": [{"year": 1}]}, "empty operator dict on field 'year'"),
    ({"$gt": 3}, "operator '$gt' where a field is expected"),
    ({"year": {"$between": [1, 2]}}, "unknown operator '$between' on field 'year'"),
    ({"year": {"$and": [{"year": 1}]}}, "unknown operator '$and' on field 'year'"),
    ({"year": {"$gt": None}}, "$gt on field 'year' cannot compare with None"),
    ({"year": {"$eq": [1, 2]}}, "must be a bool, int, float, str or None, got list"),
    ({"year": {"$eq": float("nan")}}, "is NaN"),
])
def test_grammar_refusals(where, message):
    with pytest.raises(ValueError) as e:
        W.matches(CHUNKS[0], where)
    assert message in str(e.value)
    with pytest.raises(ValueError) as e:
        W.fields_of(where)
    assert message in str(e.value)


@pytest.mark.parametrize("values, message", [
    ([["a", "b"], None, ["c"]], "field 'f' holds values of kinds ['list']"),
    (["a", 1, None], "field 'f' holds values of kinds ['int', 'str']"),
    ([True, 1], "field 'f' holds values of kinds ['bool', 'int']"),
    ([1.5, "x"], "field 'f' holds values of kinds ['float', 'str']"),
    ([1, 2 ** 63], "outside int64"),
    ([1.5, 2 ** 53 + 1], "above 2**53"),
    ([1.5, float("nan")], "holds NaN"),
])
def test_kind_refusals(values, message):
    with pytest.raises(ValueError) as e:
        W.build_column(values, "f")
    assert message in str(e.value)


@pytest.mark.parametrize("where, message", [
    ({"year": {"$gt": "2020"}}, "field 'year' is of kind int, the $gt value '2020' is of kind str"),
    ({"year": {"$eq": True}}, "field 'year' is of kind int, the $eq value True is of kind bool"),
    ({"public": {"$eq": 1}}, "field 'public' is of kind bool, the $eq value 1 is of kind int"),
    ({"company": {"$in": ["a", 3]}}, "field 'company' is of kind str, the $in value 3 is of kind int"),
    ({"score": {"$lt": "x"}}, "field 'score' is of kind number, the $lt value 'x' is of kind str"),
    ({"score": [0.5, False], "$and": [{}]}, "field 'score' is of kind number, the $in value False is of kind bool"),
])
def test_value_kind_refusals(where, message):
    with pytest.raises(ValueError) as e:
        W.compile_where(where, _columns(CHUNKS, where), n=len(CHUNKS))
    assert message in str(e.value)


def test_has_operators():
    from test_ensemble_where import WHERES
    for where in WHERES + ({}, {"tags": ["a"]}, {"a": {"b": 1}}):
        assert W.has_operators(where) is False, where
    for where, _ in EXPECTED:
        assert W.has_operators(where) is True, where
    assert W.has_operators({"a": {"$gt": 1}}) and W.has_operators({"$and": [{"a": 1}]}) and W.has_operators({"a": 1, "$or": [{"b": 2}]})


def test_key_maps_keep_order():
    ints = [-(2 ** 63), -1, 0, 1, 2 ** 63 - 1]
    col = W.build_column(ints, "i")
    assert col.kind == "int" and col.valid is None and col.keys.tolist() == ints
    floats = [-INF, -1.5, -5e-324, -0.0, +0.0, 5e-324, 1.5, INF]
    col = W.build_column(floats, "f")
    keys = col.keys.tolist()
    assert col.kind == "number" and keys[3] == keys[4], "-0.0 has the key of +0.0"
    rest = keys[:4] + keys[5:]
    assert all(a < b for a, b in zip(rest, rest[1:])), keys
    assert W.float_key(np.float64(0.0)) == 0 and W.float_key(np.array([-0.0]))[0] == 0
    mixed = W.build_column([3, 2.5, None, -(2 ** 53), 2 ** 53], "m")
    assert mixed.kind == "number" and mixed.valid.tolist() == [True, True, False, True, True]
    assert np.argsort(mixed.keys[mixed.valid]).tolist() == [2, 1, 0, 3]
    strings = ["", "A", "a", "é", "中"]
    col = W.build_column(list(reversed(strings)) + ["a"], "s")
    assert col.kind == "str" and col.values == strings and col.keys.tolist() == [4, 3, 2, 1, 0, 2]
    col = W.build_column([True, None, False], "b")
    assert col.kind == "bool" and col.keys.tolist() == [1, 0, 0] and col.valid.tolist() == [True, False, True]
    col = W.build_column([None, None], "g")
    assert col.kind is None and not col.valid.any()
    # the validity words the device reads: bit r & 31 of word r >> 5, 2 * ceil(n / 64) words, zero past n
    col = W.build_column([1 if r % 3 else None for r in range(70)], "v")
    words = col.valid_words()
    assert words.dtype == np.uint32 and words.shape == (4,)
    assert [(int(words[r >> 5]) >> (r & 31)) & 1 for r in range(128)] == [1 if (r < 70 and r % 3) else 0 for r in range(128)]


def test_compiled_shapes():
    cols = _columns(CHUNKS, {"year": 1, "company": "a", "$and": [{}]})
    one = W.compile_where({"year": {"$gte": 2020, "$lt": 2023, "$gt": 2019.5}}, cols)
    assert len(one.leaves) == 1 and one.code == [0] and one.leaves[0].tolist() == (W.LEAF_INTERVAL, 0, 2020, 2022), "orderings merge into one interval"
    assert W.compile_where({"year": {"$gt": 2 ** 63 - 1}}, cols).leaves[0].tolist() == (W.LEAF_INTERVAL, 0, 1, 0), "$gt max: the empty leaf, no overflow"
    assert W.compile_where({"year": {"$lt": -(2 ** 63)}}, cols).leaves[0].tolist() == (W.LEAF_INTERVAL, 0, 1, 0)
    assert W.compile_where({"company": {"$eq": "nobody"}}, cols).leaves[0].tolist() == (W.LEAF_INTERVAL, 0, 1, 0), "absent from the dictionary"
    four = W.compile_where({"year": {"$in": [2019, 2020, 2021, 2022]}}, cols)
    assert [int(k) for k in four.leaves["kind"]] == [W.LEAF_INTERVAL] * 4 and four.set_values.size == 0
    five = W.compile_where({"year": {"$in": [2023, 2019, 2020, 2021, 2022, 1999]}}, cols)
    assert [int(k) for k in five.leaves["kind"]] == [W.LEAF_SET] and five.set_values.tolist() == [1999, 2019, 2020, 2021, 2022, 2023]
    names = W.compile_where({"company": {"$in": ["gamma", "nobody", "alpha", "beta", "", "zz"]}}, cols)
    assert names.leaves[0].tolist() == (W.LEAF_SET, 0, 0, 4) and names.set_values.tolist() == [0, 2, 3, 5], "strings the dictionary lacks are dropped"
    assert list(five.ops) == [0] and W.compile_where({"year": {"$ne": 3}}, cols).ops.tolist() == [0, W.OP_NOT]
    chain = {"year": 2019}
    for _ in range(40):
        chain = {"$or": [{"company": "alpha"}, {"$and": [chain, {"year": {"$ne": 7}}]}]}
    deep = W.compile_where(chain, cols)
    assert deep.depth > W.MAX_DEPTH and not deep.fits_device
    want = [W.matches(md, chain) for md in CHUNKS]
    assert deep.evaluate_numpy(cols, len(CHUNKS)).tolist() == want


def test_row_mask():
    mask = W.RowMask(np.array([False, True, True, False, True]))
    assert len(mask) == 3 and list(mask) == [1, 2, 4]
    assert [r in mask for r in (-1, 0, 1, 4, 5, np.int64(2), np.int64(-1))] == [False, False, True, True, False, True, False]
    words = np.array([0b10110, 0], dtype=np.uint32)
    again = W.RowMask.from_words(words, 5)
    assert list(again) == [1, 2, 4] and len(again) == 3 and 64 not in again


METADATA = where_cases.metadata()
FAMILY = where_cases.family(METADATA)


def test_family_numpy_equals_matches():
    columns = {f: W.build_column([md.get(f) for md in METADATA], f) for f in ("page", "serial", "ratio", "company", "date", "flag", "ghost")}
    assert columns["serial"].valid is None and columns["page"].valid is not None and columns["ratio"].kind == "number"
    nontrivial, on_device, sets = 0, 0, 0
    for where in FAMILY:
        want = np.fromiter((W.matches(md, where) for md in METADATA), np.bool_, len(METADATA))
        program = W.compile_where(where, columns, n=len(METADATA))
        got = program.evaluate_numpy(columns)
        assert got.dtype == np.bool_ and np.array_equal(got, want), where
        nontrivial += 0 < int(want.sum()) < len(METADATA)
        on_device += program.fits_device
        sets += int((program.leaves["kind"] == W.LEAF_SET).any())
    share = nontrivial / len(FAMILY)
    print(f"{len(FAMILY)} filters, {nontrivial} pass a non-trivial subset ({share:.0%}), {on_device} fit the device, {sets} hold a set leaf")
    assert len(FAMILY) > 300 and 0.05 <= share <= 0.95, share
    assert on_device > 0.8 * len(FAMILY) and sets >= 10
