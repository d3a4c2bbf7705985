"""Deterministic inputs for the tests of term-rich dictionaries and of the device builder's term table (index_build.inc).

Every other dictionary of the suite stays under 37^3 distinct terms.  term_rich() is random strings of 3 to 10 symbols over 36
letters at q = 4, every third followed by a one-substitution neighbour (so that queries have more than one candidate):

  term_rich(180000)   240 000 documents, 691 501 distinct 4-grams, 10 segments, capacity (sum of len + 2) 2 039 964:
                      the device builder's table starts at 2^20 slots (capacity / 16 is below that), overflows at the 524 289th
                      term and is rebuilt once at 2^22; term ids pass 2^19, the search side's table has 2^21 slots
  term_rich(120000)   160 000 documents, 516 917 terms: the 2^20 table at load 0.49, no growth

queries(): 2 048 documents picked by RandomState(11), every odd pick longer than 4 bytes with one byte replaced.  Against
term_rich(180000) the CPU oracle gives (tests/test_term_rich_shapes_cpu.py holds the inputs to these):

  call                 rows >= 1   rows >= 2   flagged   longest row
  jaccard 0.3, k 10      0.886       0.221       0          5
  cosine 0.4, k 20       0.939       0.420       0          8
  dice 0.5, k 5          0.886       0.220       0          5

The small dictionaries stand on the edges of the builder's table once sg_debug_index_build_table_bits has shrunk it to 16 slots:
one term more than half of it, a probe chain that wraps from the last slot to slot 0, long documents and the empty term through
a repeated pass.  Used by test_term_rich_shapes_cpu.py (oracle and plain Python alone) and test_gpu_term_rich.py.  Nothing here
touches the GPU or the library.
"""
import random
from types import SimpleNamespace

import numpy as np

SYM = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
DESC = dict(ngram_size=4, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"))
CALLS = (("jaccard", 0.3, 10), ("cosine", 0.4, 20), ("dice", 0.5, 5))
MIN_ROWS_2 = (0.15, 0.30, 0.15)          # share of rows with at least two entries, per call
N_QUERIES = 2048
HIGH_TERM = 1 << 19                      # no other dictionary of the suite has a term id up here
DEFAULT_BITS = 20                        # build_on_device: the table starts at 2^20 slots, or a sixteenth of the capacity if larger


def first_overflow(bits):
    """the number of distinct non-empty terms at which a 2^bits table first flags overflow: build_intern flags when the count
    BEFORE its own increment is above mask >> 1, so 2^(bits-1) terms fit and the next one flags (16 slots: 8 fit, the 9th flags)"""
    return (1 << bits >> 1) + 1


def term_rich(n_base=180000, seed=7, every=3):
    r = np.random.RandomState(seed)
    L = r.randint(3, 11, size=n_base); sym = r.randint(0, 36, size=(n_base, 10))
    pos = r.randint(0, 1 << 30, size=n_base) % L; step = r.randint(1, 36, size=n_base)
    docs = []
    for i in range(n_base):
        s = sym[i, :L[i]]; docs.append(SYM[s].tobytes())
        if i % every == 0:                      # a one-substitution neighbour right behind its base
            v = s.copy(); v[pos[i]] = (v[pos[i]] + step[i]) % 36; docs.append(SYM[v].tobytes())
    return docs


def queries(docs, n=N_QUERIES, seed=11):
    r = np.random.RandomState(seed)
    out = []
    for j, d in enumerate(r.randint(0, len(docs), size=n)):
        q = bytearray(docs[d])
        if j % 2 == 1 and len(q) > 4:
            q[r.randint(0, len(q))] = SYM[r.randint(0, 36)]
        out.append(bytes(q))
    return out


def prefixes(qs):
    """for autocomplete: the first 2 to 5 bytes of every 8th query"""
    return [q[:2 + i % 4] for i, q in enumerate(qs[::8])]


def pack(strings):
    """list of bytes -> (uint8 blob, uint64 offsets[n + 1])"""
    offs = np.zeros(len(strings) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer(b"".join(strings), dtype=np.uint8).copy(), offs


def capacity(docs, desc=DESC):
    """what build_on_device sizes its key array by: a document's bytes plus the wrap"""
    return sum(len(d) for d in docs) + len(docs) * (len(desc["wrap"][0]) + len(desc["wrap"][1]))


def grams(docs, q=4, wrap=(b"$", b"$")):
    """-> (gram [n] uint32, doc [n] int64, segment of the doc [n_docs]): the q-grams of wrap + d + wrap, in dictionary order, for
    ASCII documents over SYM of at least one byte (none is trimmed, folded or replaced: the plain sliding window), q <= 4"""
    lens = np.array([len(d) for d in docs], dtype=np.int64) + len(wrap[0]) + len(wrap[1])
    flat = np.frombuffer(b"".join(wrap[0] + d + wrap[1] for d in docs), dtype=np.uint8).astype(np.uint32)
    start = np.zeros(len(docs) + 1, dtype=np.int64)
    start[1:] = np.cumsum(lens)
    n = np.maximum(lens - q + 1, 0)
    doc = np.repeat(np.arange(len(docs), dtype=np.int64), n)
    first = np.zeros(len(docs) + 1, dtype=np.int64)
    first[1:] = np.cumsum(n)
    at = start[doc] + np.arange(doc.size, dtype=np.int64) - first[doc]
    g = np.zeros(doc.size, dtype=np.uint32)
    for j in range(q):
        g = (g << np.uint32(8)) | flat[at + j]
    return g, doc, n


def first_appearance(g):
    """-> (term id of every gram, numbered by first appearance; number of terms)"""
    uniq, first, inv = np.unique(g, return_index=True, return_inverse=True)
    rank = np.empty(uniq.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(uniq.size)
    return rank[inv], int(uniq.size)


def plain_csr(docs, q=4, wrap=(b"$", b"$")):
    """The host CSR restated: postings, seg_off (without the slack word), n_terms, S, the (doc, cell = term * S + segment) pairs in
    store order and every document's highest term id.  Term ids by first appearance of the n-gram in dictionary order;
    segment = the document's n-gram count with repeats; list (term, segment) = the ascending docIDs, once each, padded to four
    with the last docID; seg_off in 16-byte chunks, S + 1 entries per term and one at the end."""
    g, doc, n = grams(docs, q, wrap)
    term, n_terms = first_appearance(g)
    S = int(n.max()) + 1
    cell = term * S + n[doc]
    pair = np.unique(cell * len(docs) + doc)                      # (term, segment, doc) once, ascending
    cell, doc = pair // len(docs), pair % len(docs)
    length = np.bincount(cell, minlength=n_terms * S)
    chunks = (length + 3) >> 2
    off = np.zeros(n_terms * S + 1, dtype=np.int64)
    off[1:] = np.cumsum(chunks)
    postings = np.zeros(int(off[-1]) * 4, dtype=np.uint32)
    begin = np.zeros(n_terms * S + 1, dtype=np.int64)
    begin[1:] = np.cumsum(length)
    postings[off[cell] * 4 + np.arange(cell.size) - begin[cell]] = doc
    last = doc[begin[1:][length > 0] - 1]                          # the padding: a list's last docID
    pad = chunks * 4 - length
    has = np.flatnonzero(length > 0)
    for k in (1, 2, 3):
        m = pad[has] >= k
        postings[off[has[m]] * 4 + length[has[m]] + k - 1] = last[m]
    rows = np.zeros((n_terms, S + 1), dtype=np.int64)
    rows[:, :S] = off[:-1].reshape(n_terms, S)
    rows[:, S] = off[S::S]                                         # a term's last entry: where the next term begins
    return SimpleNamespace(postings=postings, seg_off=rows.ravel().astype(np.uint32), n_terms=n_terms, S=S, doc=doc, cell=cell,
                           max_term=np.maximum.reduceat(term, first_gram(n)))


def first_gram(n):
    """the index of every document's first gram (every document has one)"""
    assert (n > 0).all()
    return np.cumsum(n) - n


def compare_csr(postings, seg_off, ref):
    """the host CSR as raw arrays against plain_csr()'s, whole; raises AssertionError naming the first differing row.  seg_off has
    one word of slack behind its n_terms x (S + 1) entries, which the builders leave 0."""
    n_rows = ref.n_terms * (ref.S + 1)
    assert seg_off.size == n_rows + 1 and seg_off[-1] == 0, ("seg_off", seg_off.size, n_rows + 1, int(seg_off[-1]))
    bad = np.flatnonzero(seg_off[:n_rows] != ref.seg_off)
    assert bad.size == 0, "seg_off row %d (term %d, segment %d) = %d, the restatement has %d" % (
        bad[0], bad[0] // (ref.S + 1), bad[0] % (ref.S + 1), seg_off[bad[0]], ref.seg_off[bad[0]])
    assert postings.size == ref.postings.size, ("postings", postings.size, ref.postings.size)
    bad = np.flatnonzero(postings != ref.postings)
    assert bad.size == 0, "posting %d (chunk %d) = %d, the restatement has %d" % (bad[0], bad[0] // 4, postings[bad[0]], ref.postings[bad[0]])


# ---- the small dictionaries of the builder's table (sg_debug_index_build_table_bits(4): 16 slots) ------------------------------
SMALL_BITS = 4
TABLE_DESC = dict(ngram_size=3, wrap=("", ""), pad="$", alphabet=("english", "numbers"))
EMPTY_PAD_DESC = dict(ngram_size=3, wrap=("", ""), pad="", alphabet=("english", "numbers"))
EMPTY_PAD_DOCS = [b"ab - c", b"--- --", b"a-b", b"   ", b"abc", b"- -", b"cab cab"]
LONG_DESC = dict(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"))


def one_term_documents(n, seed=3):
    """n distinct 3-letter documents: under TABLE_DESC a document is one trigram, so n documents are n terms"""
    r = random.Random(seed)
    out, seen = [], set()
    while len(out) < n:
        s = bytes(r.choice(SYM.tobytes()) for _ in range(3))
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def mix64(k):
    """d_mix64 (engine.hip) restated: the hash of a term key; the home slot is its low bits"""
    M = (1 << 64) - 1
    k ^= k >> 30; k = k * 0xBF58476D1CE4E5B9 & M
    k ^= k >> 27; k = k * 0x94D049BB133111EB & M
    k ^= k >> 31
    return k


def wrap_around(key_of, bits=SMALL_BITS):
    """-> (three documents whose term's home slot is the LAST slot of a 2^bits table, four others of which one has home slot 0)
    key_of: document -> term key (NGramIndex.tokenize_keys).  Seven terms: a 16-slot table takes them in one pass.  The second
    and third of the three are interned, and found again, past the end of the table: in slot 0 or behind it."""
    mask = (1 << bits) - 1
    last, zero, other = [], [], []
    for d in one_term_documents(400, seed=5):
        h = mix64(key_of(d)) & mask
        if h == mask and len(last) < 3:
            last.append(d)
        elif h == 0 and len(zero) < 1:
            zero.append(d)
        elif 4 <= h <= mask - 4 and len(other) < 3:
            other.append(d)
    assert len(last) == 3 and len(zero) == 1 and len(other) == 3
    return last, zero + other


def empty_pad_documents():
    """the empty-pad dictionary of test_device_index_build_is_identical_to_host_build — foreign runes vanish from an n-gram, an
    n-gram of foreign runes alone is the EMPTY term (key 0, kept beside the table) — and four one-term documents: that dictionary
    alone has seven terms and the empty one, which a 16-slot table takes in one pass; these make it twelve"""
    return EMPTY_PAD_DOCS * 40 + [b"xyz", b"k9q", b"mno", b"w0w"]


def long_documents():
    """the documents of test_device_index_build_takes_long_documents — four of them the long tokeniser's: three above 128 n-grams,
    one of five distinct n-grams above 144 runes — among 300 short ones, under LONG_DESC"""
    rnd = random.Random(5)
    long_doc = bytes(rnd.choice(SYM.tobytes()) for _ in range(400))
    longs = [b"short", long_doc, long_doc[:129], long_doc[100:300] * 3, b"abc" * 200]
    shorts = [bytes(rnd.choice(SYM.tobytes()) for _ in range(rnd.randint(4, 9))) for _ in range(300)]
    return shorts[:90] + longs[:2] + shorts[90:200] + longs[2:4] + shorts[200:] + longs[4:]


SORT_KEY_DESC = dict(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "russian", "$"))


def refusal_sort_key():
    """a 65 000-byte document of random runes over 68 letters (about 41 000 distinct trigrams, as many segments) and 80 000
    three-letter documents, each with a middle trigram of its own: terms x segments passes the 32-bit sort key — about 4.8 x 10^9;
    test_term_rich_shapes_cpu.py counts it.  (Not for the host builder: its seg_off would be 20 GB.)"""
    rnd = random.Random(9)
    letters = [chr(c) for c in SYM.tobytes()] + [chr(c) for c in range(0x430, 0x450)]          # a-z 0-9 а-я
    n = len(letters)
    long_doc = b""
    while len(long_doc) < 64998:
        long_doc += rnd.choice(letters).encode("utf-8")
    long_doc += b"q" * (65000 - len(long_doc))
    return [long_doc] + [(letters[i // n // n] + letters[i // n % n] + letters[i % n]).encode("utf-8") for i in range(80000)]


REPEATS_A_TERM = b"a-a+"      # under LONG_DESC: $a$ a$a $a$ a$$ — the tokeniser keeps an n-gram once, so b"aaaa" repeats nothing; the
#                               foreign runes become the pad, and two different n-grams become one term
