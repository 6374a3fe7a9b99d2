"""Seeded chunk metadata and an ENUMERATED family of operator filters over it, shared by tests/test_where_grammar.py (NumPy route against
``where.matches``) and tests/test_gpu_where.py (the device against both).  Nothing here is random at test time: one seed, fixed lists.

Fields: ``page`` int with 10 % missing; ``serial`` int, every row has it (no validity bitmap); ``ratio`` floats and ints mixed (kind
number) with 15 % missing, -0.0 / +0.0 / an infinity among them; ``company`` str (24 tenants, some non-ASCII) with 5 % missing; ``date`` ISO
date strings, every row; ``flag`` bool with 30 % missing; ``ghost``: no row has it."""
import random

COMPANIES = ["acme", "Acme", "zeekr", "lotus", "é-corp", "中石化", "", "b", "ba", "bb"] + [f"tenant{i:02d}" for i in range(14)]
SCALAR_OPS = ("$eq", "$ne", "$gt", "$gte", "$lt", "$lte")


def metadata(n=300, seed=24):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        md = {"doc_id": f"d{i}", "serial": rng.randrange(0, 2000), "date": f"20{rng.randrange(18, 26):02d}-{rng.randrange(1, 13):02d}-{rng.randrange(1, 29):02d}"}
        if rng.random() >= 0.10:
            md["page"] = rng.randrange(1, 61)
        if rng.random() >= 0.15:
            md["ratio"] = rng.choice([0.5, -0.0, 0.0, 3, -7, 2.25, -1e-300, 1e300, float("inf"), rng.uniform(-5, 5), rng.randrange(-4, 5)])
        if rng.random() >= 0.05:
            md["company"] = rng.choice(COMPANIES)
        if rng.random() >= 0.30:
            md["flag"] = rng.random() < 0.4
        out.append(md)
    return out


def _bounds(present, kind):
    """Comparison values below, at, between and above the present values of a field."""
    vs = sorted(set(present))
    lo, mid, hi = vs[0], vs[len(vs) // 2], vs[-1]
    if kind == "int":
        return [lo - 1, lo, mid, mid + 0.5, hi, hi + 1, float("-inf")]
    if kind == "number":
        finite = [v for v in vs if abs(v) < 1e200]
        return [-1e308, lo, finite[len(finite) // 2], 0, 0.123456, 2, finite[-1], float("inf"), 2 ** 60 + 1]
    if kind == "str":
        return ["", lo, mid, mid + "!", hi, hi + "z", "\U0010ffff"]
    return [False, True]


def family(mds, seed=24):
    """[where, ...]: every scalar operator on every kind at the bounds above; $in / $nin of 1, 4, 5 and 200 values with absent members
    and None; missing-field filters; $and / $or trees of depth 1 to 4 over those."""
    rng = random.Random(seed)
    kinds = {"page": "int", "serial": "int", "ratio": "number", "company": "str", "date": "str", "flag": "bool"}
    leaves = []
    for field, kind in kinds.items():
        present = [md[field] for md in mds if field in md]
        for x in _bounds(present, kind):
            for op in SCALAR_OPS:
                leaves.append({field: {op: x}})
        leaves.append({field: {"$eq": None}})
        leaves.append({field: {"$ne": None}})
        vs = sorted(set(present))
        absent = {"int": [-10 ** 6, 10 ** 6, 2.5], "number": [1234.5, -99], "str": ["nobody", "zzz"], "bool": []}[kind]
        for size in (1, 4, 5, 200):
            take = [vs[(j * 7) % len(vs)] for j in range(max(1, size - len(absent)))][:size] + absent
            take = take[:size] if kind != "bool" else take[:2]
            leaves.append({field: {"$in": take}})
            leaves.append({field: {"$nin": take + [None]}})
            leaves.append({field: list(take) + [None], "$and": [{}]})   # the plain-list shorthand, inside an operator filter
    leaves.append({"page": {"$gte": 10, "$lte": 40}})
    leaves.append({"page": {"$gt": 40, "$lt": 10}})
    leaves.append({"date": {"$lte": "2022-06-15", "$gt": "2019"}, "page": {"$gte": 3}})
    leaves.append({"serial": {"$gte": 100, "$lt": 1500, "$ne": 777}})
    leaves.append({"company": "zeekr", "flag": {"$ne": True}})
    leaves.append({"ghost": {"$ne": 1}})
    leaves.append({"ghost": {"$eq": None}})
    leaves.append({"ghost": {"$gt": "a"}})
    leaves.append({"ghost": {"$in": [1, None]}})
    leaves.append({"ghost": {"$nin": [1]}})

    def tree(depth):
        if depth == 0:
            return rng.choice(leaves)
        return {rng.choice(("$and", "$or")): [tree(depth - 1) for _ in range(rng.choice((1, 2, 2, 3)))]}

    trees = [tree(d) for d in (1, 2, 3, 4) for _ in range(15)]
    return leaves + trees
