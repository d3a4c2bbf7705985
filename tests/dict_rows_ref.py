"""A numpy restatement of the materialise step's rules (include/suggest_hip.h, sg_dictionary_rows) and the shapes
its tests run: id rows, counts, a row geometry and the dictionary's lines in, (text, text_offs, needed, outside) out.  It shares
nothing with the library: every result of the step, host or device, is compared with it byte for byte."""
import numpy as np

COUNT_FLAG_MIN = 0xFFFFFFF0          # counts from here up are SG_COUNT_* flags: the row has no entries
POISON_ID = 0xA5A5A5A5               # what sg_debug_poison(1) leaves in the id slots past a row's count


def pack(lines):
    offs = np.zeros(len(lines) + 1, dtype=np.uint64)
    if lines:
        offs[1:] = np.cumsum([len(b) for b in lines], dtype=np.uint64)
    blob = np.frombuffer(b"".join(lines), dtype=np.uint8).copy()
    return blob, offs


def materialise(ids, counts, blob, offs, row=None, row_offs=None, slots=None):
    """-> (text u8, text_offs[slots + 1] u64, needed, outside).  Fixed stride `row`, or ragged row_offs[n_rows + 1].  Row i has
    min(counts[i], its length) entries, none where counts[i] >= 0xFFFFFFF0; every other slot is empty and its id is not looked
    at; an entry whose id is >= n_docs is empty and counted in `outside`."""
    ids = np.asarray(ids, dtype=np.uint32).reshape(-1)
    counts = np.asarray(counts, dtype=np.uint32).reshape(-1).astype(np.int64)
    offs = np.asarray(offs, dtype=np.uint64).astype(np.int64)
    n_docs, n_rows = len(offs) - 1, len(counts)
    slots = ids.size if slots is None else int(slots)
    s = np.arange(slots, dtype=np.int64)
    if row_offs is None:
        row = int(row)
        r = s // row if row else np.full(slots, n_rows, dtype=np.int64)
        in_row = r < n_rows
        r = np.minimum(r, max(n_rows - 1, 0))
        pos = s - r * row
        row_len = np.full(slots, row, dtype=np.int64)
    else:
        ro = np.asarray(row_offs, dtype=np.uint64).astype(np.int64)
        assert len(ro) == n_rows + 1 and np.all(ro[1:] >= ro[:-1])
        r = np.searchsorted(ro[:n_rows], s, side="right") - 1        # the last row that begins at or before the slot
        in_row = r >= 0
        r = np.maximum(r, 0)
        in_row &= s < ro[r + 1] if n_rows else False
        pos = s - ro[r] if n_rows else s
        row_len = ro[r + 1] - ro[r] if n_rows else s * 0
    if n_rows == 0:
        entry = np.zeros(slots, dtype=bool)
    else:
        c = counts[r]
        entry = in_row & (c < COUNT_FLAG_MIN) & (pos < np.minimum(c, row_len))
    assert ids.size >= slots
    idv = np.where(entry, ids[:slots].astype(np.int64), 0)
    out = entry & (idv >= n_docs)
    take = entry & ~out
    idv = np.where(take, idv, 0)
    length = np.where(take, offs[idv + 1] - offs[idv], 0) if n_docs else np.zeros(slots, dtype=np.int64)
    text_offs = np.zeros(slots + 1, dtype=np.int64)
    np.cumsum(length, out=text_offs[1:])
    total = int(text_offs[slots])
    nz = length > 0
    src0 = np.repeat(offs[idv[nz]], length[nz])
    within = np.arange(total, dtype=np.int64) - np.repeat(text_offs[:-1][nz], length[nz])
    text = np.asarray(blob, dtype=np.uint8)[src0 + within] if total else np.zeros(0, dtype=np.uint8)
    return text, text_offs.astype(np.uint64), total, int(out.sum())


def check(got_text, got_offs, ref):
    """the step's result against materialise()'s, byte for byte (AssertionError where they differ)"""
    text, text_offs = ref[0], ref[1]
    got_offs = np.asarray(got_offs, dtype=np.uint64)
    assert got_offs.shape == text_offs.shape, "text_offs: %s entries, expected %s" % (got_offs.shape, text_offs.shape)
    bad = np.nonzero(got_offs != text_offs)[0]
    assert bad.size == 0, "text_offs[%d] = %d, expected %d" % (bad[0], got_offs[bad[0]], text_offs[bad[0]])
    got_text = np.asarray(got_text, dtype=np.uint8)[:text.size]
    assert got_text.size == text.size, "text: %d bytes, expected %d" % (got_text.size, text.size)
    bad = np.nonzero(got_text != text)[0]
    assert bad.size == 0, "text[%d] = %d, expected %d" % (bad[0], got_text[bad[0]], text[bad[0]])


# ---- the step's shapes ----
def step_lines():
    """203 strings: lengths 0 .. 40 in a scrambled order (197 of them), then 63, 64, 65, 255, 4 096 and 70 001 bytes"""
    rng = np.random.default_rng(2024)
    lens = [(i * 23 + 7) % 41 for i in range(197)] + [63, 64, 65, 255, 4096, 70001]
    return [rng.integers(1, 256, size=n, dtype=np.uint8).tobytes() for n in lens]


STEP_SHAPES = [(1, 1), (15, 1), (16, 1), (17, 1), (3, 7), (257, 5), (1, 65536)]


def count_values(row):
    return [0, 1, max(row - 1, 0), row, row + 1, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF]


def step_cases():
    """[(name, n_rows, row, variant)]: shapes with fewer than 8 rows come in as many variants as it takes for the rows to meet
    all 8 count values"""
    out = []
    for n_rows, row in STEP_SHAPES:
        for v in range(-(-8 // n_rows) if n_rows < 8 else 1):
            out.append(("%dx%d_v%d" % (n_rows, row, v), n_rows, row, v))
    return out


def step_rows(n_rows, row, variant, n_docs):
    """-> (ids[n_rows, row] u32, counts[n_rows] u32): row i's count is count_values(row)[(variant * n_rows + i) % 8]; ids within
    the count are random docIDs, past it poison, n_docs and 2^32 - 1 in turn"""
    rng = np.random.default_rng(n_rows * 1000003 + row * 101 + variant)
    vals = count_values(row)
    counts = np.array([vals[(variant * n_rows + i) % 8] for i in range(n_rows)], dtype=np.uint32)
    ids = rng.integers(0, n_docs, size=(n_rows, row), dtype=np.uint32)
    past = np.array([POISON_ID, n_docs, 0xFFFFFFFF], dtype=np.uint32)
    for i in range(n_rows):
        c = int(counts[i])
        n = 0 if c >= COUNT_FLAG_MIN else min(c, row)
        ids[i, n:] = past[(np.arange(row - n) + i) % 3]
    return ids, counts
