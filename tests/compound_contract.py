"""The contract of the rows chained into compound loci (include/ribbit_hip.h) in plain Python: the clipped rows ordered by
(s', e', index), one sweep that keeps `reach`.  And a brute force for small sets (the chains are the connected components of
"lie at most gap apart"), the sets on which the tests compare an implementation with the contract, and what follows from the
contract (tests/test_compound.py, tests/test_compound_gpu.py)."""
import numpy as np

import best_contract
from best_contract import I32_MAX, I32_MIN, clipped

FIELDS = ("bases", "start", "end", "rows", "classes", "switches", "overlaps", "first", "pad")
GAPS = (0, 1, 7, 100, I32_MAX)
LENGTHS = (0, 1, 64, 300, 4100)


def record_compounds(length, intervals, labels, gap):
    """-> (the chains as dicts with the keys FIELDS, by ascending start; members)"""
    assert len(intervals) == len(labels) and gap >= 0
    order = sorted((s, e, i) for i, (s, e) in enumerate(clipped(length, intervals)) if s < e)
    chains, reach = [], 0
    for k, (s, e, i) in enumerate(order):
        if k == 0 or s - reach > gap:
            chains.append(dict(bases=0, start=s, end=e, rows=0, classes=0, switches=0, overlaps=0, first=k, pad=0, labels=set()))
            reach = e
        else:
            c = chains[-1]
            c["switches"] += int(labels[i]) != int(labels[order[k - 1][2]])
            c["overlaps"] += s < reach
            reach = max(reach, e)
        c = chains[-1]
        c["end"] = reach
        c["rows"] += 1
        c["bases"] += e - s
        c["labels"].add(int(labels[i]))
    for c in chains:
        c["classes"] = len(c.pop("labels"))
    return chains, [i for _, _, i in order]


def as_dicts(compounds):
    """a COMPOUND_DT array as the dicts record_compounds returns"""
    return [{f: int(c[f]) for f in FIELDS} for c in compounds]


def brute_force(length, intervals, labels, gap):
    """the chains as the connected components of the non-empty rows under "max(s'_a, s'_b) - min(e'_a, e'_b) <= gap", with
    classes, bases and switches recomputed naively per component: [(start, end, rows, bases, classes, switches)] by start"""
    rows = [(s, e, i) for i, (s, e) in enumerate(clipped(length, intervals)) if s < e]
    assert len(rows) <= 200
    parent = list(range(len(rows)))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    for a in range(len(rows)):
        for b in range(a):
            if max(rows[a][0], rows[b][0]) - min(rows[a][1], rows[b][1]) <= gap:
                parent[find(a)] = find(b)
    parts = {}
    for a in range(len(rows)):
        parts.setdefault(find(a), []).append(rows[a])
    out = []
    for part in parts.values():
        part.sort()
        lab = [int(labels[i]) for _, _, i in part]
        out.append((part[0][0], max(e for _, e, _ in part), len(part), sum(e - s for s, e, _ in part), len(set(lab)),
                    sum(a != b for a, b in zip(lab, lab[1:]))))
    return sorted(out)


def against_brute_force(chains):
    return [(c["start"], c["end"], c["rows"], c["bases"], c["classes"], c["switches"]) for c in chains]


def edge_case_sets(length):
    """[(intervals, labels)]: the sets of best_contract.edge_case_sets with labels that repeat, nested rows where reach decides
    (at gaps 39, 40 and 209 the set (10,200),(20,30),(240,260) is two chains, one, one; the last row lies 40 behind the reach and
    210 behind the row before it), duplicates with different labels, and the int32 limits as labels of one chain"""
    sets = [(iv, [(3 * i) % 4 - 1 for i in range(len(iv))]) for iv in best_contract.edge_case_sets(length)]
    sets.append(([(10, 200), (20, 30), (240, 260)], [1, 2, 2]))
    sets.append(([(240, 260), (20, 30), (10, 200)], [7, 7, 7]))
    sets.append(([(10, 200), (20, 30), (31, 40), (100, 120), (200, 201), (209, 230)], [0, 1, 0, 1, 0, 0]))
    sets.append(([(20, 30)] * 4 + [(25, 35)] * 3, [5, 4, 5, 3, 9, 9, 8]))
    sets.append(([(5, 9), (9, 14), (14, 20), (20, 21)], [I32_MIN, -1, 0, I32_MAX]))
    sets.append(([(14, 20), (5, 9), (20, 21), (9, 14), (5, 9)], [I32_MAX, I32_MIN, I32_MIN, I32_MAX, -1]))
    return sets


def random_record(rs, t, n_labels):
    """(length, intervals, labels): the rows as best_contract.random_record draws them, labels from n_labels values around 0"""
    length, iv = best_contract.random_record(rs, t)
    return length, iv, rs.randint(-(n_labels // 2), n_labels - n_labels // 2, len(iv))


def check_properties(length, intervals, labels, compounds, members):
    """what follows from the contract, checked on a result however it was made (compounds: a COMPOUND_DT array)"""
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    s, e = np.maximum(iv[:, 0], 0), np.minimum(iv[:, 1], length)
    full = np.flatnonzero(s < e)
    want = full[np.lexsort((full, e[full], s[full]))]
    members = np.asarray(members)
    assert np.array_equal(members, want)                              # a permutation of the non-empty rows in (s', e', i) order
    c = compounds
    assert (c["pad"] == 0).all() and (c["rows"] >= 1).all()
    first = np.concatenate([[0], np.cumsum(c["rows"], dtype=np.int64)])
    assert np.array_equal(c["first"], first[:-1]) and first[-1] == len(members)      # the chains tile members
    assert (c["classes"] - 1 <= c["switches"]).all() and (c["switches"] <= c["rows"] - 1).all()
    assert np.array_equal(c["classes"] == 1, c["switches"] == 0)
    assert (c["overlaps"] <= c["rows"] - 1).all() and (c["overlaps"] >= 0).all()
    assert c["bases"].sum() == (e[full] - s[full]).sum()
    if len(c):
        assert np.array_equal(c["start"], s[members[first[:-1]]])
        assert (c["start"][1:] > c["end"][:-1]).all()                    # (more than gap >= 0 behind the chain before)
        lab = np.asarray(labels)[members]
        differs = np.concatenate([[0], np.cumsum(lab[1:] != lab[:-1])])      # switches: label changes inside the chains
        inside = differs[first[1:] - 1] - differs[first[:-1]]
        assert np.array_equal(c["switches"], inside)
