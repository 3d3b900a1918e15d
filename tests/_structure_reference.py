"""Host restatement of the two structure builders of include/gml.h (gml_structure_from_rows / gml_structure_from_keys) in numpy and
itertools: the keys of every node are enumerated in the slot order of its row (pairwise: slot j <-> spin j, slot u = the field;
multi-body: the order of gml_multi_keys -- by size, then the other spins in lexicographic order, GraphicalModelLearning.jl:94-104),
grouped by sorted key, and every group decided as the header states it.  TEST INFRASTRUCTURE ONLY: nothing of the product imports it."""
import itertools

import numpy as np

EXCLUDED, FREE, PENALISED = 0, 1, 2


def node_keys(n, order, u):
    """the keys (u, S') of node u's parameter slots, 0-based, in slot order"""
    if order == 2:
        return [(u,) if j == u else (u, j) for j in range(n)]
    others = [i for i in range(n) if i != u]
    return [(u,) + comb for s in range(1, order + 1) for comb in itertools.combinations(others, s - 1)]


def params_per_node(n, order):
    return len(node_keys(n, order, 0))


def key_groups(n, order):
    """{sorted key: [(u, slot) of its members, ascending u]}"""
    groups = {}
    for u in range(n):
        for j, k in enumerate(node_keys(n, order, u)):
            groups.setdefault(tuple(sorted(k)), []).append((u, j))
    return groups


def keep_key(values, rule, threshold):
    """the decision of one key from its members' entries (ascending u); a NaN compares false"""
    if rule == "mean":
        total = 0.0
        for v in values:  # added in ascending u, then / |S|: the operations of the term assembly
            total = total + float(v)
        return abs(total / float(len(values))) >= threshold
    hits = [abs(float(v)) >= threshold for v in values]
    return all(hits) if rule == "all" else any(hits)


def structure_from_rows(rows, n, order, threshold, rule="mean", keep=FREE, drop=EXCLUDED, field=FREE):
    """(uint8 [n, P], kept) as gml_structure_from_rows defines them"""
    rows = np.asarray(rows, dtype=np.float64)
    S = np.zeros((n, params_per_node(n, order)), dtype=np.uint8)
    kept = 0
    for key, members in key_groups(n, order).items():
        if len(key) == 1:
            (u, j), = members
            S[u, j] = field
            continue
        if rule == "row":
            for u, j in members:
                k = bool(abs(float(rows[u, j])) >= threshold)
                S[u, j] = keep if k else drop
                kept += k
            continue
        k = bool(keep_key([rows[u, j] for u, j in members], rule, threshold))
        for u, j in members:
            S[u, j] = keep if k else drop
        kept += len(members) * k
    return S, kept


def structure_from_keys(keys0, n, order, listed=PENALISED, other=EXCLUDED, field=FREE):
    """uint8 [n, P] as gml_structure_from_keys defines it; keys0: 0-based tuples (sets of 1 .. order spins)"""
    groups = key_groups(n, order)
    S = np.full((n, params_per_node(n, order)), other, dtype=np.uint8)
    for key, members in groups.items():
        if len(key) == 1:
            (u, j), = members
            S[u, j] = field
    for k in keys0:
        for u, j in groups[tuple(sorted(int(i) for i in k))]:
            S[u, j] = listed
    return S
