"""tests/mixed_shapes.py — the rules of a mixed batch in numpy — held against its own checkers on the shapes the GPU test runs, and
the checkers shown to refuse what they are there to refuse.  No library call."""
import numpy as np
import pytest

import mixed_shapes as ms


@pytest.mark.parametrize("name,config_of,ks", ms.shapes(), ids=[s[0] for s in ms.shapes()])
def test_rules_hold_on_every_shape(name, config_of, ks):
    n_configs = len(ks)
    perm, start = ms.permutation(config_of, n_configs)
    ms.check_permutation(perm, start, config_of, n_configs)
    # the counting statement equals a stable sort by config number
    assert np.array_equal(perm, np.argsort(np.asarray(config_of, dtype=np.int64), kind="stable").astype(np.uint32))
    assert np.array_equal(np.diff(start.astype(np.int64)), np.bincount(np.asarray(config_of, dtype=np.int64), minlength=n_configs))
    ro = ms.row_offsets(config_of, ks)
    ms.check_row_offsets(ro, config_of, ks)
    pos = ms.scatter_positions(config_of, ks, perm, start)
    ms.check_scatter_positions(pos, config_of, ks, start)
    rb = ms.row_bases(start, ks)
    assert np.all(rb % 4 == 0) and np.all(np.diff(rb.astype(np.int64)) >= 0)
    # rows that carry (query number, slot) come back in caller order
    grouped = np.zeros(int(rb[-1]), dtype=np.uint64)
    for j, i in enumerate(perm.tolist()):
        g = int(config_of[i])
        k = int(ks[g])
        at = int(rb[g]) + (j - int(start[g])) * k
        grouped[at:at + k] = (np.uint64(i) << np.uint64(32)) + np.arange(k, dtype=np.uint64)
    rows = ms.scatter(config_of, ks, perm, start, grouped)
    for i in range(len(config_of)):
        k = int(ks[int(config_of[i])])
        assert np.array_equal(rows[int(ro[i]):int(ro[i + 1])], (np.uint64(i) << np.uint64(32)) + np.arange(k, dtype=np.uint64))


def test_grouped_offsets_and_blob_follow_the_permutation():
    rng = np.random.RandomState(5)
    lens = np.array([0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 0], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    blob = rng.randint(1, 255, int(offs[-1])).astype(np.uint8)
    config_of = rng.randint(0, 4, len(lens)).astype(np.uint32)
    perm, start = ms.permutation(config_of, 4)
    go = ms.grouped_offsets(offs, perm)
    gb = ms.grouped_blob(blob, offs, perm)
    assert go[0] == 0 and go[-1] == offs[-1] and len(gb) == int(offs[-1])
    for j, i in enumerate(perm.tolist()):
        assert np.array_equal(gb[int(go[j]):int(go[j + 1])], blob[int(offs[i]):int(offs[i + 1])])


def test_the_checker_fails_on_a_swap_inside_a_group():
    config_of = ms.sizes_batch()[ms.order(ms.sizes_batch(), "shuffled")]
    perm, start = ms.permutation(config_of, len(ms.GROUP_SIZES))
    ms.check_permutation(perm, start, config_of, len(ms.GROUP_SIZES))
    bad = perm.copy()
    lo = int(start[3])                      # two entries of one group (64 queries) change places
    bad[lo + 5], bad[lo + 6] = perm[lo + 6], perm[lo + 5]
    with pytest.raises(AssertionError, match="caller's order"):
        ms.check_permutation(bad, start, config_of, len(ms.GROUP_SIZES))
    bad = perm.copy()                       # a query in another config's group
    bad[int(start[2])], bad[int(start[3])] = perm[int(start[3])], perm[int(start[2])]
    with pytest.raises(AssertionError, match="another config"):
        ms.check_permutation(bad, start, config_of, len(ms.GROUP_SIZES))
    bad = perm.copy()
    bad[0] = bad[1]
    with pytest.raises(AssertionError, match="permutation"):
        ms.check_permutation(bad, start, config_of, len(ms.GROUP_SIZES))


def test_the_checker_fails_on_row_offsets_off_by_one():
    config_of = np.array([0, 1, 1, 0, 2], dtype=np.uint32)
    ks = [3, 7, 1]
    ro = ms.row_offsets(config_of, ks)
    assert ro.tolist() == [0, 3, 10, 17, 20, 21]
    ms.check_row_offsets(ro, config_of, ks)
    bad = ro.copy()
    bad[2] += 1
    with pytest.raises(AssertionError, match="row 1"):
        ms.check_row_offsets(bad, config_of, ks)
    bad = ro.copy()
    bad[-1] -= 1
    with pytest.raises(AssertionError, match="row 4"):
        ms.check_row_offsets(bad, config_of, ks)
    perm, start = ms.permutation(config_of, 3)
    pos = ms.scatter_positions(config_of, ks, perm, start)
    ms.check_scatter_positions(pos, config_of, ks, start)
    pos[1] = (pos[1][0], pos[1][1] + 1, pos[1][2])
    with pytest.raises(AssertionError):
        ms.check_scatter_positions(pos, config_of, ks, start)


def test_orders_keep_the_multiset():
    base = ms.sizes_batch()
    for how in ms.ORDERS:
        o = ms.order(base, how)
        assert np.array_equal(np.sort(o), np.arange(len(base))), how
    rr = base[ms.order(base, "round_robin")]
    assert rr[:5].tolist() == [1, 2, 3, 4, 5]          # (config 0 has no query)
