"""The rules of a mixed batch (sg_suggest_batch_mixed; suggest_amd/csrc/mixed_batch.inc) restated in numpy, and the
shapes the tests run them on.  Nothing here touches the library: tests/test_mixed_shapes_cpu.py holds the restatement against its
own checkers, tests/test_gpu_mixed.py holds the device against it word for word.

  perm          grouped position j -> the caller's number of the query there: ascending config number, and within a config the
                caller's order (a stable sort of the query numbers by config number)
  group_start   [n_configs + 1]: first grouped position of every config (an exclusive sum of the configs' query counts)
  grouped offs  [n_q + 1]: an exclusive sum of the queries' byte lengths in grouped order; the grouped blob holds query perm[j]
                at [offs[j], offs[j + 1])
  row_offs      [n_q + 1]: row i of the caller starts at the sum of the k of the queries before it (caller order)
  row_base      [n_configs + 1]: first slot of a group's dense rows in the grouped rows; a group starts at a multiple of four slots
  scatter       grouped row j (group g, k_g slots from row_base[g] + (j - group_start[g]) * k_g) -> caller slots from
                row_offs[perm[j]]
"""
import numpy as np

MAX_CONFIGS = 256


def permutation(config_of, n_configs):
    """-> (perm, group_start) by counting, not by sorting: every config's queries are listed in caller order, config after config"""
    config_of = np.asarray(config_of, dtype=np.int64)
    assert config_of.size == 0 or (config_of.min() >= 0 and config_of.max() < n_configs)
    perm, start = [], [0]
    for g in range(n_configs):
        members = np.flatnonzero(config_of == g)          # ascending: caller order
        perm.extend(members.tolist())
        start.append(len(perm))
    return np.array(perm, dtype=np.uint32), np.array(start, dtype=np.uint32)


def grouped_offsets(offs, perm):
    offs = np.asarray(offs, dtype=np.uint64)
    lens = (offs[1:] - offs[:-1])[np.asarray(perm, dtype=np.int64)]
    return np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64)


def grouped_blob(blob, offs, perm):
    blob = np.asarray(blob, dtype=np.uint8)
    parts = [blob[int(offs[i]):int(offs[i + 1])] for i in np.asarray(perm, dtype=np.int64)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def row_offsets(config_of, ks):
    k_of = np.asarray(ks, dtype=np.uint64)[np.asarray(config_of, dtype=np.int64)]
    return np.concatenate([[0], np.cumsum(k_of, dtype=np.uint64)]).astype(np.uint64)


def row_bases(group_start, ks):
    base = [0]
    for g, k in enumerate(ks):
        n = int(group_start[g + 1]) - int(group_start[g])
        base.append(base[-1] + ((n * int(k) + 3) & ~3))
    return np.array(base, dtype=np.uint64)


def scatter_positions(config_of, ks, perm, group_start):
    """-> [(first grouped slot, first caller slot, slots)] for every grouped position j"""
    ro, rb = row_offsets(config_of, ks), row_bases(group_start, ks)
    out = []
    for j, i in enumerate(np.asarray(perm, dtype=np.int64)):
        g = int(config_of[i])
        k = int(ks[g])
        out.append((int(rb[g]) + (j - int(group_start[g])) * k, int(ro[i]), k))
    return out


def scatter(config_of, ks, perm, group_start, grouped_rows):
    """the caller's ragged rows from the groups' dense rows (any dtype)"""
    ro = row_offsets(config_of, ks)
    out = np.zeros(int(ro[-1]), dtype=np.asarray(grouped_rows).dtype)
    for src, dst, k in scatter_positions(config_of, ks, perm, group_start):
        out[dst:dst + k] = grouped_rows[src:src + k]
    return out


# ---- checkers: each states a property on its own terms, so that the restatement above is held against something ----

def check_permutation(perm, group_start, config_of, n_configs):
    perm = np.asarray(perm, dtype=np.int64)
    config_of = np.asarray(config_of, dtype=np.int64)
    n_q = config_of.size
    assert perm.shape == (n_q,), "perm has one entry per query"
    assert np.array_equal(np.sort(perm), np.arange(n_q)), "perm is a permutation of the query numbers"
    assert len(group_start) == n_configs + 1 and int(group_start[0]) == 0 and int(group_start[-1]) == n_q, "group_start spans the batch"
    for g in range(n_configs):
        lo, hi = int(group_start[g]), int(group_start[g + 1])
        assert lo <= hi, "group_start ascends"
        members = perm[lo:hi]
        assert np.all(config_of[members] == g), "group %d holds a query of another config" % g
        assert np.all(members[1:] > members[:-1]), "group %d does not keep the caller's order" % g


def check_row_offsets(row_offs, config_of, ks):
    row_offs = np.asarray(row_offs)
    assert row_offs.shape == (len(config_of) + 1,) and int(row_offs[0]) == 0, "row_offs has n_q + 1 entries from 0"
    for i, g in enumerate(config_of):
        assert int(row_offs[i + 1]) - int(row_offs[i]) == int(ks[int(g)]), "row %d does not have its config's k slots" % i


def check_scatter_positions(pos, config_of, ks, group_start):
    """the caller's slots are covered exactly once; the grouped slots of no two rows overlap and stay inside their group"""
    total = int(sum(int(ks[int(g)]) for g in config_of))
    seen = np.zeros(total, dtype=np.int32)
    rb = row_bases(group_start, ks)
    taken = np.zeros(int(rb[-1]), dtype=np.int32)
    for src, dst, k in pos:
        seen[dst:dst + k] += 1
        taken[src:src + k] += 1
    assert np.all(seen == 1), "a caller slot is written twice or never"
    assert taken.size == 0 or taken.max() <= 1, "two rows share a grouped slot"
    for g in range(len(ks)):
        assert np.all(taken[int(rb[g]):int(rb[g]) + (int(group_start[g + 1]) - int(group_start[g])) * int(ks[g])] == 1), "group %d's rows are not dense" % g


# ---- shapes ----

GROUP_SIZES = (0, 1, 63, 64, 65, 257)          # wavefront and workgroup boundaries, an unused config


def order(config_sorted, how, seed=7):
    """the same multiset of config numbers in another caller order: "sorted", "reversed", "round_robin", "shuffled" -> an index array
    into the sorted batch (apply it to the queries as well)"""
    n = len(config_sorted)
    if how == "sorted":
        return np.arange(n)
    if how == "reversed":
        return np.arange(n)[::-1].copy()
    if how == "shuffled":
        return np.random.RandomState(seed).permutation(n)
    assert how == "round_robin"
    config_sorted = np.asarray(config_sorted)
    queues = [list(np.flatnonzero(config_sorted == g)) for g in range(int(config_sorted.max()) + 1 if n else 0)]
    out = []
    while any(queues):
        for q in queues:
            if q:
                out.append(q.pop(0))
    return np.array(out, dtype=np.int64)


ORDERS = ("sorted", "reversed", "round_robin", "shuffled")


def sizes_batch():
    """config numbers of a batch with GROUP_SIZES queries per config, sorted by config"""
    return np.concatenate([np.full(n, g, dtype=np.uint32) for g, n in enumerate(GROUP_SIZES)])


def shapes():
    """[(name, config_of, ks)] — the CPU test runs every rule on each"""
    out = []
    base = sizes_batch()
    ks6 = [1, 10, 64, 65, 100, 5]
    for how in ORDERS:
        out.append(("sizes_" + how, base[order(base, how)], ks6))
    out.append(("one_query", np.array([2], dtype=np.uint32), [3, 4, 5]))
    out.append(("one_config", np.zeros(70, dtype=np.uint32), [10]))
    c256 = np.concatenate([np.arange(256), [17]]).astype(np.uint32)
    out.append(("256_configs", c256[order(c256, "shuffled", seed=3)], list(range(1, 257))))
    out.append(("empty", np.zeros(0, dtype=np.uint32), [10, 20]))
    return out
