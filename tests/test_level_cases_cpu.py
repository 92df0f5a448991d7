"""The references of tests/test_partition_levels.py and tests/test_scan_levels.py without a GPU (tests/level_cases.py): the numpy
statements of Partition + folds, of FoldSelect over general runs and of GROUP BY agree with the oracle on small inputs of the same
shape, and the O(n) checker of a stable partition accepts the true positions and rejects each way of being slightly wrong."""
import numpy as np
import pytest

import level_cases as lc
from helpers import oracle_run


def _oracle_outputs(text, cols, named):
    res = oracle_run(text, cols)
    return {name: lc.out(res, node) for name, node in named.items()}


@pytest.mark.parametrize("mode", ["positions", "scatters only, keys inside", "scatters only, keys outside", "EPS rows", "one pass"])
def test_partition_reference_is_what_the_oracle_computes(mode):
    rng = np.random.default_rng(5)
    n, pmin, pcount = 30011, 1000, 1 << 20
    keys = rng.integers(pmin, pmin + pcount, n)
    keys[rng.integers(0, n, n // 4)] = rng.integers(pmin, pmin + 50, n // 4)             # ties, also across far-apart slots
    if mode == "scatters only, keys outside":
        keys[rng.integers(0, n, 500)] = rng.integers(-5000, pmin + 1, 500)
        keys[rng.integers(0, n, 500)] = rng.integers(pmin + pcount, pmin + pcount + 9000, 500)
        keys[:3] = [np.iinfo(np.int64).min + 7, np.iinfo(np.int64).max - 7, pmin]
    if mode == "one pass":
        pmin, pcount = 0, 200
        keys = rng.integers(-3, 230, n)
    vals = rng.integers(-10 ** 9, 10 ** 9, n)
    flags = (rng.integers(0, 3, n) != 0) if mode == "EPS rows" else None
    text, named = lc.partition_program(pmin, pcount, flags is not None, mode in ("positions", "EPS rows", "one pass"))
    cols = lc.partition_cols(keys, vals, rng, flags)
    got = _oracle_outputs(text, cols, named)
    ref = lc.partition_reference(keys, vals, flags, pmin, pcount)
    for name in named:
        assert np.array_equal(got[name], ref[name]), name
    if lc.POS in named:
        assert lc.stable_partition_error(lc.buckets(keys, pmin, pcount), flags, pos=got[lc.POS], slots=got.get(lc.SLOTS)) is None


def test_buckets_do_not_wrap_at_the_ends_of_int64():
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    keys = np.array([lo, lo + 1, -1, 0, 1, 5, 6, 7, hi - 1, hi], np.int64)
    for pmin, pcount in ((5, 1), (lo, 10), (lo, hi), (hi - 3, 2), (-1, hi), (0, 1 << 45)):
        want = [min(max(int(k) - pmin, 0), pcount) for k in keys]
        assert lc.buckets(keys, pmin, pcount).tolist() == want, (pmin, pcount)


def test_the_checker_accepts_the_stable_partition_and_nothing_near_it():
    rng = np.random.default_rng(6)
    n = 5000
    bucket = rng.integers(0, 40, n)
    valid = rng.integers(0, 5, n) != 0
    slots = np.flatnonzero(valid)
    local = np.argsort(bucket[slots], kind="stable")
    pos = np.empty(len(slots), np.int64)
    pos[local] = np.arange(len(slots))
    order = slots[local]
    assert lc.stable_partition_error(bucket, valid, pos=pos) is None
    assert lc.stable_partition_error(bucket, valid, pos=pos, slots=slots) is None
    assert lc.stable_partition_error(bucket, valid, order=order) is None
    assert lc.stable_partition_error(bucket, None, order=np.argsort(bucket, kind="stable")) is None

    # two rows of the same bucket swapped: still a permutation, still in bucket order -- only stability is lost
    r = int(np.flatnonzero(bucket[order][1:] == bucket[order][:-1])[0])
    bad = pos.copy()
    a, b = np.searchsorted(slots, order[r]), np.searchsorted(slots, order[r + 1])
    bad[a], bad[b] = pos[b], pos[a]
    assert "slot order" in lc.stable_partition_error(bucket, valid, pos=bad)
    swapped = order.copy()
    swapped[r], swapped[r + 1] = order[r + 1], order[r]
    assert "slot order" in lc.stable_partition_error(bucket, valid, order=swapped)

    # a position handed out twice (and one never)
    bad = pos.copy()
    bad[10] = bad[11]
    assert "twice" in lc.stable_partition_error(bucket, valid, pos=bad)
    dup = order.copy()
    dup[10] = dup[11]
    assert "twice" in lc.stable_partition_error(bucket, valid, order=dup)

    # a single inversion: two neighbouring ranks of different buckets exchanged
    r = int(np.flatnonzero(bucket[order][1:] != bucket[order][:-1])[0])
    bad = pos.copy()
    a, b = np.searchsorted(slots, order[r]), np.searchsorted(slots, order[r + 1])
    bad[a], bad[b] = pos[b], pos[a]
    assert "descend" in lc.stable_partition_error(bucket, valid, pos=bad)

    # an EPS row that carries a rank: one more position than valid rows / an EPS slot among the ranked rows
    eps = int(np.flatnonzero(~valid)[0])
    with_eps = np.sort(np.append(slots, eps))
    assert "non-EPS" in lc.stable_partition_error(bucket, valid, pos=np.append(pos, len(pos)), slots=with_eps)
    assert "positions for" in lc.stable_partition_error(bucket, valid, pos=np.append(pos, len(pos)))
    stolen = order.copy()
    stolen[0] = eps
    assert lc.stable_partition_error(bucket, valid, order=stolen) is not None
    assert lc.stable_partition_error(bucket, valid, order=np.append(order, eps)) is not None
    # a position outside 0 .. m-1
    bad = pos.copy()
    bad[0] = len(pos)
    assert "outside" in lc.stable_partition_error(bucket, valid, pos=bad)


def test_general_run_select_reference_is_what_the_oracle_computes():
    rng = np.random.default_rng(7)
    n = 40000
    ctl = np.sort(rng.integers(0, 900, n)).astype(np.int32)
    ctl[rng.integers(0, n, n // 3)] = rng.integers(0, 900, n // 3)
    ctl[20000:26000] = 17                                                       # a long run
    flags = (rng.integers(0, 50, n) != 0).astype(np.int8)
    data = rng.integers(0, 3, n).astype(np.int8)
    text, named = lc.general_select_program()
    res = oracle_run(text, {"t.c": ctl, "t.f": flags, "t.d": data})
    slots, values = lc.general_select_reference(ctl, flags != 0, data)
    assert np.array_equal(lc.out(res, named["hits"]), values)
    assert np.array_equal(lc.out(res, named["offset"]), slots - values)
    assert np.array_equal(lc.out(res, named["data"]), data[values])
    assert np.any(slots != values)


@pytest.mark.parametrize("shape", ["distinct", "runs of 7", "one run", "descent at the end", "shuffled"])
def test_group_by_reference_is_what_the_oracle_computes(shape):
    rng = np.random.default_rng(8)
    n = 20001
    keys = lc.sorted_keys(n, shape) if shape != "shuffled" else rng.permutation(lc.sorted_keys(n, "runs of 7"))
    vals = rng.integers(-10 ** 12, 10 ** 12, n)
    text, named = lc.group_by_program(1 << 40)
    res = oracle_run(text, {"t.k": keys, "t.v": vals})
    ref = lc.group_by_reference(keys, vals)
    for name, node in named.items():
        assert np.array_equal(lc.out(res, node), ref[name]), name
