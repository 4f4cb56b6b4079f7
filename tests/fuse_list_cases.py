"""Synthetic sub-lists for the two fuse kernels (csrc/hybrid_fuse.hpp; DESIGN.md sections 13 - 15): lists no search of the index
would produce - unsorted, with ids that repeat inside a list, holes anywhere, foreign ids, negative / cancelling / huge / infinite
scores - and, per kind, the check that the case reaches what it is built for (its AIM), asserted on the ORACLE's answer before any
device result is looked at. numpy only; nothing of the package is imported, so the CPU suite builds and checks every case.

A case is (scores [nq, R, lmax] float32, ids [nq, R, lmax] int64) for an index of n rows whose row 0 has id id_base. A hit's rank is
its slot: holes and foreign ids keep their slot.

The order of a run's sum (ascending (r, j)) shows only where the sum is inexact: under RRF, whose terms 1 / (c + j + 1) are, and
under `wide_range` scores. Float32 scores of one magnitude, times weights of a few bits, sum exactly in double in any order.

Left out on purpose: NaN scores and lists that hold both infinities (or +inf under a weight of 0.0). Their fused value is NaN, and
the oracle's `sorted` defines no order for NaN; `plus_inf` therefore puts +inf into lists 0 and 1 only, whose weights are never 0.
"""
import numpy as np

LIST_KINDS = ("disjoint", "identical", "rotated", "repeats", "holes", "empty", "few")
SCORE_KINDS = ("plain", "negative", "cancel", "signed_zero", "subnormal", "huge", "plus_inf", "tied", "wide_range")
GROUPED_KINDS = ("abab", "aabb", "split", "repeats", "empty")
W_MIXED = [1.0, 0.5, 0.25, 0.75, 0.125, 0.875, 0.375, 0.0]   # a 1.0 and a 0.0 (request 7)
W_ONES = [1.0] * 8                                            # +x and -x of two lists cancel exactly
FEW = 5                                                       # distinct ids of a `few` query
# (R, lmax): R * lmax is in the range of every width the sort network runs at, 2 .. 1024
WIDTHS = ((1, 1), (2, 1), (3, 1), (1, 5), (3, 5), (5, 6), (7, 9), (8, 16), (1, 128), (3, 43), (5, 100), (8, 65), (8, 128))


def sort_width(R, lmax):
    w = 2
    while w < R * lmax:
        w <<= 1
    return w


def limit_sets(R, lmax):
    """every list at lmax; a mixed vector with a 1 and values below lmax (the same thing where lmax is 1)"""
    mixed = [1 if r == 0 else max(1, (lmax * (r + 1)) // (R + 1)) for r in range(R)]
    return [[lmax] * R] + ([mixed] if mixed != [lmax] * R else [])


def foreign_ids(n, id_base):
    """ids that are no row of the index: padding, the id in front of the first row, the one behind the last, one 2^33 further, and
    (with an id_base) a small positive id"""
    return [-1, id_base - 1, id_base + n, id_base + n + 2 ** 33] + ([5] if id_base > 5 else [])


def empty_query(nq):
    return nq // 2


def build_ids(kind, nq, R, lmax, n, id_base, seed):
    """local rows first, then + id_base; -1 and foreign ids are put in last"""
    rng = np.random.default_rng(seed)
    rows = np.full((nq, R, lmax), -1, np.int64)
    for q in range(nq):
        perm = rng.permutation(n)
        if kind in ("disjoint", "holes", "empty"):
            for r in range(R):
                for j in range(lmax):
                    if j * R + r < n:
                        rows[q, r, j] = perm[j * R + r]
        elif kind == "identical":
            rows[q, :, :] = perm[:lmax]
        elif kind == "rotated":
            for r in range(R):
                rows[q, r] = np.roll(perm[:lmax], -r)
        elif kind == "few":
            rows[q] = perm[:FEW][rng.integers(0, FEW, (R, lmax))]
        elif kind == "repeats":
            anchor = perm[0]
            if q % 3 == 0:                       # ONE id in every slot: a single run of R * lmax
                rows[q] = anchor
                continue
            shared = perm[1:9]
            for r in range(R):
                own = perm[20 + 3 * r: 23 + 3 * r]                      # three ids no other list holds
                tokens = np.repeat(shared, rng.integers(2, 6, len(shared)))   # every shared id 2 to 5 times
                seq = np.resize(rng.permutation(tokens), lmax)
                seq[:2] = anchor                                          # the anchor twice in front of EVERY list: a run above R
                if lmax >= 7:
                    seq[2:6] = np.repeat(own[:2], 2)                      # two of them twice each, next to themselves
                    seq[6] = own[2]                                       # ... the third once: in a zero-weight list it fuses to 0.0
                rows[q, r] = seq
        else:
            raise AssertionError(kind)
    ids = np.where(rows >= 0, rows + id_base, -1)
    if kind == "holes":
        bad = foreign_ids(n, id_base)
        for q in range(nq):
            for r in range(R):
                for j in (sorted({0, lmax // 2, lmax - 1} if r == 0 else {lmax // 2, lmax - 1} if lmax > 1 else set())):
                    ids[q, r, j] = bad[(q * R + r) % len(bad)] if j == lmax // 2 else -1
    if kind == "empty":
        bad = foreign_ids(n, id_base)
        q = empty_query(nq)
        ids[q] = np.asarray(bad, np.int64)[rng.integers(0, len(bad), (R, lmax))]
    return ids


def build_scores(kind, ids, seed):
    """scores for the given ids; `cancel` looks at them, the other kinds do not"""
    rng = np.random.default_rng(seed + 1000)
    nq, R, lmax = ids.shape
    u = rng.random(ids.shape)
    if kind == "plain":          # positive, best first
        s = -np.sort(-(0.05 + 0.9 * u), axis=2)
    elif kind == "negative":     # in (-1, 0), best first
        s = -np.sort(0.01 + 0.98 * u, axis=2)
    elif kind == "signed_zero":
        s = np.where(u < 0.5, 0.0, -0.0)
    elif kind == "subnormal":
        s = np.where(rng.random(ids.shape) < 0.5, 1.0, -1.0) * (0.5 + u) * 1e-42
    elif kind == "huge":
        s = np.where(rng.random(ids.shape) < 0.8, 1.0, -1.0) * (1e38 + 2e38 * u)
    elif kind == "tied":
        s = np.where(u < 0.5, 0.5, 0.25)
    elif kind == "wide_range":   # signed magnitudes from 1e-30 to 1e30: float32 scores of ONE magnitude sum exactly in double in any
        s = np.where(rng.random(ids.shape) < 0.5, 1.0, -1.0) * 10.0 ** (60.0 * u - 30.0)   # order - these do not, so the order of a run's sum shows
    elif kind == "plus_inf":
        s = -np.sort(-(0.05 + 0.9 * u), axis=2)
        s[:, :2, :3] = np.inf
    elif kind == "cancel":
        # an even id cancels: inside a list its occurrences pair up as +x, -x (one list, one weight: exact under any weights), an
        # unpaired one is +x in an even list and -x in an odd one (exact under equal weights); x depends on the id alone. Odd ids
        # keep signed scores of their own. The pairing is made over the whole list: use it with limits equal to lmax.
        s = (u - 0.4).astype(np.float64)
        for q in range(nq):
            for r in range(R):
                seen = {}
                for j in range(lmax):
                    i = int(ids[q, r, j])
                    if i < 0 or i % 2:
                        continue
                    x = 0.125 + (i % 997) / 1024.0
                    seen.setdefault(i, []).append(j)
                    s[q, r, j] = x if len(seen[i]) % 2 else -x
                for i, js in seen.items():
                    if len(js) % 2 and r % 2:
                        s[q, r, js[-1]] = -s[q, r, js[-1]]
    else:
        raise AssertionError(kind)
    s = s.astype(np.float32)
    assert not np.isnan(s).any() and not np.isneginf(s).any()
    return s


def build(kind, nq, R, lmax, n, id_base=0, seed=0, scores="plain"):
    ids = build_ids(kind, nq, R, lmax, n, id_base, seed)
    return build_scores(scores, ids, seed), ids


def cut(sc, ids, q, limits):
    """query q's R lists cut at the limits: what the oracle's fuse_query takes"""
    return [(sc[q, r, :limits[r]], ids[q, r, :limits[r]]) for r in range(len(limits))]


def restrict_to(ids, keep):
    """ids that are not in `keep` (a view's ids) become padding and keep their slot"""
    return np.where(np.isin(ids, keep), ids, -1)


# ---- the aims: what a case must reach, measured on the oracle's FULL answer (k = every slot) ---------------------------------------
def measure(full, sc, ids, q, limits, n, id_base):
    """full: hybrid_oracle.fuse_query(cut(...), ..., k = R * lmax)[0] of query q -> what the answer shows"""
    fused, out_ids, _lv, bits = full
    m = int((out_ids >= 0).sum())
    assert (out_ids[:m] >= 0).all() and (out_ids[m:] == -1).all() and np.isneginf(fused[m:]).all() and not np.isnan(fused[:m]).any()
    assert ((out_ids[:m] >= id_base) & (out_ids[:m] < id_base + n)).all()                # no foreign id is a hit
    R = len(limits)
    slots = {}                                                                          # id -> [(r, j)] inside the limits
    valid = 0
    for r in range(R):
        for j in range(limits[r]):
            i = int(ids[q, r, j])
            if id_base <= i < id_base + n:
                slots.setdefault(i, []).append((r, j))
                valid += 1
    assert sorted(slots) == sorted(out_ids[:m].tolist())                                # the heads are the distinct valid ids
    f, o = fused[:m], out_ids[:m]
    tie = (f[1:] == f[:-1]) if m > 1 else np.zeros(0, bool)
    assert (o[1:][tie] > o[:-1][tie]).all()                                             # a fused tie comes out id-ascending
    zero = f == 0.0
    nlists = np.array([len({r for r, _ in slots[int(i)]}) for i in o], np.int64)
    count = np.array([len(slots[int(i)]) for i in o], np.int64)
    assert all(int(bits[p]) == sum(1 << r for r in {r for r, _ in slots[int(o[p])]}) for p in range(m))
    return {"heads": m, "valid": valid, "ties": int(tie.sum()), "negative": bool((f < 0).any()), "all_negative": bool(m and (f < 0).all()),
            "zero": int(zero.sum()), "zero_cancelled": bool((zero & (count >= 2)).any()), "zero_single_list": bool((zero & (nlists == 1) & (count == 1)).any()),
            "inf": int(np.isposinf(f).sum()), "huge": bool((np.abs(f[np.isfinite(f)]) > 1e30).any()),
            "tiny": bool(((np.abs(f) < 1e-37) & (f != 0.0)).any()), "longest_run": int(count.max()) if m else 0,
            "max_lists": int(nlists.max()) if m else 0, "slots": slots, "fused": f, "ids": o}


def assert_list_aim(kind, ms, R, lmax, limits, k=None, ranker="rrf"):
    """ms: measure() of every query of the case, in order"""
    nq = len(ms)
    wide = any(l >= 2 for l in limits)
    if kind == "disjoint":
        for m in ms:
            assert m["heads"] == m["valid"] > 0 and m["longest_run"] == 1           # every valid slot a head of its own
            if ranker == "rrf" and sum(1 for l in limits if l >= 1) >= 2:
                assert m["ties"] >= 1                                                # rank j of two lists ties: the id decides
    elif kind == "identical":
        for m in ms:
            assert m["heads"] == max(limits) and m["max_lists"] == R and m["longest_run"] == R
    elif kind == "rotated":
        for m in ms:
            assert m["longest_run"] <= R and m["heads"] >= max(limits)
            if R > 1 and min(limits) == lmax:
                assert m["max_lists"] == R
                if lmax >= R:                                                        # the same id at R different ranks
                    assert any(len({j for _, j in v}) == R for v in m["slots"].values())
    elif kind == "repeats":
        assert ms[0]["heads"] == 1 and ms[0]["longest_run"] == sum(limits)           # ONE run over every slot
        for q, m in enumerate(ms):
            if q % 3 and wide:
                assert m["longest_run"] > R                                          # a run longer than R: an id repeats inside a list
    elif kind == "holes":
        for m in ms:
            assert m["longest_run"] <= 1 and m["heads"] == m["valid"]
            if ranker == "rrf":                                                      # the holes did not shift a rank: 1 / (c + slot + 1)
                for i, fv in zip(m["ids"], m["fused"]):
                    (_r, j), = m["slots"][int(i)]
                    assert fv == 1.0 / (60.0 + j + 1)
    elif kind == "empty":
        e = empty_query(nq)
        assert ms[e]["heads"] == 0 and all(m["heads"] > 0 for q, m in enumerate(ms) if q != e)
    elif kind == "few":
        for m in ms:
            assert 1 <= m["heads"] <= FEW
            if k is not None and k > FEW:
                assert m["heads"] < k                                                # padding behind the hits
    else:
        raise AssertionError(kind)


def assert_score_aim(score, ms, R, weights, norm, list_kind):
    """what a score kind must show in the oracle's answer under the weighted ranker"""
    zero_weight = any(w == 0.0 for w in weights[:R])
    equal = len(set(weights[:R])) == 1
    if score == "negative" and norm == "none":
        assert all(m["negative"] for m in ms)
        if not zero_weight:
            assert all(m["all_negative"] for m in ms)
    elif score == "cancel" and norm == "none":
        if list_kind == "repeats":
            assert any(m["zero_cancelled"] for m in ms)                              # +x and -x inside a list: any weights
            if zero_weight:
                assert any(m["zero_cancelled"] and m["zero_single_list"] and m["ties"] for m in ms)   # both kinds of 0.0, tied
        elif equal and R % 2 == 0:
            assert all(m["zero_cancelled"] for m in ms)                              # +x and -x across lists: equal weights
    elif score == "signed_zero" and norm == "none":
        assert all(m["zero"] == m["heads"] for m in ms)
    elif score == "subnormal" and norm == "none":
        assert any(m["tiny"] for m in ms)
    elif score == "huge":
        assert all(m["huge"] for m in ms)
    elif score == "plus_inf":
        assert all(m["inf"] >= 1 for m in ms) and any(m["inf"] >= 2 and m["ties"] for m in ms)
    elif score == "wide_range" and norm == "none":
        assert all((np.abs(m["fused"]) > 1e15).any() for m in ms)
    elif score == "tied":
        assert any(m["ties"] for m in ms)


# ---- lists for the grouped fuse ----------------------------------------------------------------------------------------------------
def groupings(n):
    rows = np.arange(n)
    return {"own": rows.astype(np.int32), "one": np.full(n, 7, np.int32), "mod7": (rows % 7).astype(np.int32), "fam20": (rows // 20 + 100).astype(np.int32)}


KS = ((1, 1), (10, 3), (4, 32), (128, 1), (1, 128))
GROUPED_WIDTHS = ((2, 1), (3, 5), (7, 9), (3, 43), (8, 128))


def grouped_limits(R, lmax, s):
    """limits in GROUPS, limits[r] * s <= 128, mixed"""
    top = max(1, min(128 // s, max(1, lmax // 2)))
    return [max(1, top - (r % 3)) for r in range(R)]


def build_grouped_ids(kind, nq, R, lmax, group_of, s, limits, seed):
    """ids of an index with id_base 0 whose row i lies in group group_of[i]"""
    n = len(group_of)
    if kind in ("repeats", "empty"):
        return build_ids(kind, nq, R, lmax, n, 0, seed)
    rng = np.random.default_rng(seed)
    groups = np.unique(group_of)
    members = {int(g): np.flatnonzero(group_of == g) for g in groups}
    ids = np.full((nq, R, lmax), -1, np.int64)
    for q in range(nq):
        for r in range(R):
            if kind == "abab":     # consecutive slots alternate between two groups: slot j is run j + 1
                ab = rng.choice(groups, 2, replace=False) if len(groups) > 1 else [groups[0], groups[0]]
                for j in range(lmax):
                    mem = members[int(ab[j % 2])]
                    ids[q, r, j] = mem[(j // 2) % len(mem)]
                continue
            j, run, prev = 0, 0, None
            while j < lmax:
                run += 1
                g = int(rng.choice(groups))
                if g == prev and len(groups) > 1:
                    g = int(groups[(np.searchsorted(groups, g) + 1) % len(groups)])
                prev = g
                length = s + 2 if run == limits[r] else int(rng.integers(1, s + 4))   # the last run in front of the cut: longer than s
                mem = rng.permutation(members[g])
                for t in range(min(length, lmax - j)):
                    ids[q, r, j + t] = mem[t % len(mem)]
                if kind == "split" and length >= 3 and j + 1 < lmax:
                    ids[q, r, j + 1] = (-1, n + 5)[run % 2]                           # a hole / a foreign id inside the run
                j += length
    return ids


def groups_and_members(raw, k, s):
    """(distinct groups, smallest member count) of one query's oracle answer (fused, ids, levels, bits, groups)"""
    g = raw[4][raw[1] >= 0]
    if not len(g):
        return 0, 0
    _, counts = np.unique(g, return_counts=True)
    return len(counts), int(counts.min())
