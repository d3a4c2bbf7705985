"""The shapes the edit-distance tests share (tests/test_edit_rows_cpu.py: the host-resident handle; tests/test_gpu_edit_rank.py:
the kernels): one small dictionary that holds every kind of string the kernels can go wrong on, queries of every length at which
the code takes another path, and id rows over them.  Everything is derived from fixed seeds."""
import numpy as np

import edit_ref as ref

QUERY_RUNES = (0, 1, 63, 64, 65, 127, 128, 129, 1000)      # 64: the last bit of the word; 65: the long kernel; 128 / 129: block carry
CAND_RUNES = (0, 1, 64, 300)
ROW_SLOTS = (1, 64, 65, 1024, 1025, 4096)                  # the lane stride; the re-rank's switch of routes
FLAGS = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC)
POISON_ID = 0xA5A5A5A5


def _text(rng, n, alphabet):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


def colliding_runes(n, like=ord("a"), lo=0x100, hi=0x3000):
    """n caseless-enough runes above ASCII that hash to the Peq slot of `like`"""
    out = [r for r in range(lo, hi) if ref.peq_hash(r) == ref.peq_hash(like) and ref.runes(chr(r), True) == (r,) and not 0xD800 <= r < 0xE000]
    assert len(out) >= n
    return out[:n]


def dense_strings(n=60, seed=21):
    rng = np.random.default_rng(seed)
    return [_text(rng, int(rng.integers(0, 10)), "abc").encode() for _ in range(n)]


def build():
    """-> dict(lines=[bytes], named={name: docID}, dense=[docIDs])"""
    rng = np.random.default_rng(20)
    lines, named = [], {}

    def add(name, b):
        named[name] = len(lines)
        lines.append(b if isinstance(b, bytes) else b.encode("utf-8"))
    add("empty", b"")
    add("one", b"q")
    add("c64", _text(rng, 64, "abcdeXYZ "))
    add("c300", _text(rng, 300, "abAB "))
    dense = []
    for b in dense_strings():
        dense.append(len(lines))
        lines.append(b)
    add("two_byte", "\u041d\u0438\u0432\u0430 \u0428\u0435\u0432\u0440\u043e\u043b\u0435 \u043f\u0440\u0438\u0432\u0435\u0442")
    add("three_byte", "\u30c8\u30e8\u30bf \u30ab\u30ed\u30fc\u30e9 \u2103\u212a")                     # U+212A KELVIN SIGN folds to k: 3 bytes to 1
    add("four_byte", "a\U0001f600b\U0001f601\U0001f600c")
    add("width", "\u0130stanbul K\u0130LO \u212ak")                    # U+0130 folds to i: 2 bytes to 1
    add("bad_start", b"\xffnissan")
    add("bad_middle", b"nis\xc3san\xe2\x82")
    add("bad_end", b"nissan\x80")
    add("bad_only", b"\xff\xfe")
    add("fffd", "\ufffd\ufffd")
    cjk = "".join(chr(0x4E00 + i) for i in range(64))
    add("full64", cjk)
    add("full64_rot", cjk[7:] + cjk[:7])
    add("full64_gap", cjk[:20] + "xyz" + cjk[25:60])
    col = colliding_runes(8)
    add("collide", "".join(chr(r) for r in col[:5]) + "a")
    add("collide_perm", "a" + "".join(chr(r) for r in reversed(col[:5])))
    add("collide_absent", "".join(chr(r) for r in col[3:8]) + "zzz")      # three runes of the slot that the query does not hold
    for w in ("nissan", "Nissan Micra", "toyota", "TOYOTA COROLLA", "toyota corolla", "ATOYOT", "niva", "nsisan", "chevrolet niva"):
        add(w, w)
    add("long4096", _text(rng, 4096, "abc"))
    add("truncated_last", b"abc\xf0\x9f\x98")                            # the blob's last bytes: a 4-byte rune cut short
    return dict(lines=lines, named=named, dense=dense, collide=col)


def query_of(n_runes, seed=0):
    """a query of exactly n_runes runes: a small alphabet (transpositions and ties abound), upper case and a few multi-byte runes"""
    rng = np.random.default_rng(100 + seed + n_runes)
    q = _text(rng, n_runes, ["a", "b", "c", "A", "B", " ", "\u041d", "\u30c8", "\U0001f600", "\u212a"])
    assert len(ref.decode(q.encode())) == n_runes
    return q.encode()


def length_cases(shapes):
    """every query length against every candidate length -> (queries, ids [n, 4], counts)"""
    cand = [shapes["named"][k] for k in ("empty", "one", "c64", "c300")]
    queries = [query_of(n) for n in QUERY_RUNES]
    ids = np.tile(np.array(cand, dtype=np.uint32), (len(queries), 1))
    return queries, ids, np.full(len(queries), 4, dtype=np.uint32)


def dense_cases(shapes):
    """a few thousand pairs over a three-letter alphabet"""
    queries = dense_strings(60, seed=22)
    ids = np.tile(np.array(shapes["dense"], dtype=np.uint32), (len(queries), 1))
    return queries, ids, np.full(len(queries), ids.shape[1], dtype=np.uint32)


def special_cases(shapes):
    """multi-byte runes, invalid bytes, the truncated rune at the blob's end, width-changing folds, the full Peq table, colliding
    and absent runes: every special line as a query against every special line"""
    nm = shapes["named"]
    keys = ["two_byte", "three_byte", "four_byte", "width", "bad_start", "bad_middle", "bad_end", "bad_only", "fffd", "full64", "full64_rot",
            "full64_gap", "collide", "collide_perm", "collide_absent", "nissan", "Nissan Micra", "TOYOTA COROLLA", "toyota corolla", "ATOYOT", "nsisan",
            "truncated_last", "empty"]
    cand = np.array([nm[k] for k in keys], dtype=np.uint32)
    queries = [shapes["lines"][int(c)] for c in cand] + [b"niss\xf0\x9f\x98", b"\xf0\x9f\x98", "k\u0130".encode(), "\u212a\u0130".encode()]
    ids = np.tile(cand, (len(queries), 1))
    return queries, ids, np.full(len(queries), len(cand), dtype=np.uint32)


def short_ids(shapes):
    """the docIDs random rows draw from: everything but the 4 096-rune line"""
    return np.array([i for i in range(len(shapes["lines"])) if i != shapes["named"]["long4096"]], dtype=np.uint32)


def row_cases(shapes, row, seed=0):
    """rows of `row` slots: counts 0, 1 and row, a clipped count above row, a flagged row between ordinary ones, scores that descend
    with ties; slots past a count hold ids that must not be read (one of them >= n_docs) -> (queries, ids, scores, counts)"""
    rng = np.random.default_rng(300 + row + seed)
    pool = short_ids(shapes)
    counts = np.array([row, 0, 1, FLAGS[row % 4], row, row + 3, max(1, row // 2)], dtype=np.uint32)
    n = len(counts)
    ids = pool[rng.integers(0, len(pool), (n, row))].astype(np.uint32)
    scores = -np.sort(-np.round(rng.random((n, row)), 1), axis=1)
    for i, c in enumerate(counts):
        k = 0 if c >= ref.COUNT_FLAG_MIN else min(int(c), row)
        if c < ref.COUNT_FLAG_MIN:
            ids[i, k:] = [(POISON_ID, len(shapes["lines"]), 0xFFFFFFFF)[j % 3] for j in range(row - k)]
    queries = [query_of((5, 9, 63, 64, 12, 70, 3)[i], seed=row) for i in range(n)]
    return queries, ids, scores, counts


def ragged_cases(shapes, seed=0):
    """ragged rows as suggest_batch_mixed returns them, with a spare tail that belongs to no row"""
    rng = np.random.default_rng(400 + seed)
    ks = [1, 7, 300, 2, 64, 0, 9, 1100]
    ro = np.concatenate([[0], np.cumsum(ks)]).astype(np.uint64)
    slots = int(ro[-1]) + 5
    pool = short_ids(shapes)
    ids = pool[rng.integers(0, len(pool), slots)].astype(np.uint32)
    scores = np.round(rng.random(slots), 1)
    counts = np.array([1, 3, 300, 0xFFFFFFFF, 70, 0, 9, 1100], dtype=np.uint32)
    queries = [query_of((4, 8, 16, 5, 65, 3, 0, 10)[i], seed=7) for i in range(len(ks))]
    return queries, ids, scores, counts, ro, slots
