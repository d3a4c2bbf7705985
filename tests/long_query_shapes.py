"""Deterministic inputs for the long-query kernel's tests (sg_long_kernel: long_tokenize, long_query, the slot lock).

Two families.  dense(): a big dictionary over five symbols, so that a cardinality segment holds hundreds of documents, most
documents repeat a term and posting lists pass 256 raw entries.  limits(): small dictionaries whose queries stand on both
sides of every limit of the kernel's slot (65 536 n-gram windows, 65 536 bytes, the hash table at its largest).

Used by test_long_query_shapes_cpu.py (the oracle alone: the inputs reach the edges they are made for) and by
test_gpu_long_queries.py (the device against the oracle).  Nothing here touches the GPU.
"""
import numpy as np

MAX_A = 128                      # SG_MAX_A: n-grams of the wavefront kernel's tables
MAX_RUNES = 144                  # SG_MAX_RUNES
WRAP_MAX = 8                     # SG_WRAP_MAX
LONG_MAX = 65536                 # SG_LONG_MAX_TERMS: windows, and bytes, of a slot of the long-query kernel

COUNT_PANIC, COUNT_DEADLOCK, COUNT_TOO_LONG = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD

DENSE_DESC = dict(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"))
DENSE_CALLS = (("jaccard", 0.5, 10), ("cosine", 0.3, 10), ("dice", 0.4, 100), ("overlap", 0.6, 7), ("cosine", 0.2, 70))
FLAG_CALL = ("jaccard", 0.95, 5)
PAGING = ("dice", 0.4)            # suggest_all: few enough candidates to page through three at a time
FOREIGN = b"efghijklmnopqrstuvwxyz"

# Secondary entries (a docID twice in a row: a document that repeats a term) score at their segment's
# threshold, so they show only in rows that reach down to it — never in the rows of a text over "abcd ", which are full of
# better documents.  These queries are a document's first `length` symbols followed by `foreign` random foreign letters
# (and "z" up to 150 symbols): most of their n-grams are in no document, the candidates are few, and a repeated docID shows
# in the rows of at least one of DENSE_CALLS.  (doc, length, foreign) were found by trying 30 000 such queries of dense()
# against the oracle; test_long_query_shapes_cpu.py checks what they are here for.
DILUTED = ((16591, 103, 30), (9109, 57, 5), (425, 73, 20), (525, 21, 20), (1627, 73, 0), (10724, 114, 20), (8995, 87, 5), (4819, 121, 60),
           (19853, 123, 45), (14867, 53, 150), (2484, 24, 100), (792, 113, 60), (18762, 99, 45))
TABLE_A_MAX = 40


def text(rnd, n, letters):
    """n symbols of `letters` (bytes: one-byte symbols; str: runes, UTF-8 encoded)"""
    pick = rnd.randint(0, len(letters), size=int(n))
    if isinstance(letters, bytes):
        return np.frombuffer(letters, np.uint8)[pick].tobytes()
    return "".join(letters[i] for i in pick).encode("utf-8")


def runes_of(q):
    return len(q.decode("utf-8"))            # (strict: the generators only make valid UTF-8)


def windows(desc, q):
    """n-gram windows of the wrapped, trimmed text before the dedup (G of long_tokenize); 0: no window loop is run"""
    t = (desc["wrap"][0].encode() + q.lower() + desc["wrap"][1].encode()).decode("utf-8").strip(" ")
    return max(0, len(t) - desc["ngram_size"] + 1) if len(t) > desc["ngram_size"] else 0


def is_long(ora, desc, q, autocomplete=False):
    """What d_tokenize gives up on (returns -1), from the oracle's tokens and the rune count alone: an ASCII text of more than
    144 runes with its wrap, any other text whose runes pass 144 - 8 before the closing wrap, or more than 128 distinct n-grams."""
    w0 = len(desc["wrap"][0])
    w1 = 0 if autocomplete else len(desc["wrap"][1])
    if all(b < 0x80 for b in q):
        if w0 + len(q) + w1 > MAX_RUNES:
            return True
    elif w0 + runes_of(q) > MAX_RUNES - WRAP_MAX:
        return True
    return len(ora.tokenize(q, autocomplete)) > MAX_A


def long_set(ora, desc, queries, autocomplete=False):
    return {i for i, q in enumerate(queries) if is_long(ora, desc, q, autocomplete)}


def interleave(rnd, few, many):
    """`few` spread between `many`, deterministic; -> (list, positions of `few` in it)"""
    at = sorted(rnd.choice(len(few) + len(many), size=len(few), replace=False).tolist())
    out, rest = [None] * (len(few) + len(many)), iter(many)
    for p, q in zip(at, few):
        out[p] = q
    return [next(rest) if q is None else q for q in out], at


# ---- 1. the dense dictionary ---------------------------------------------------------------------------------------------
def dense(n_docs=20000, seed=11):
    """-> dict: docs, queries (long and short mixed), flag_queries (for FLAG_CALL), paging (queries for suggest_all), prefixes
    (long autocomplete prefixes), families (docIDs of documents that share a 160-symbol stem), diluted (the DILUTED queries)"""
    rnd = np.random.RandomState(seed)
    letters = b"abcd "
    lens = rnd.randint(20, 221, size=n_docs)
    pool = text(rnd, lens.sum(), letters)
    ends = np.cumsum(lens)
    docs = [pool[int(e - n):int(e)] for e, n in zip(ends, lens)]
    # families: ten documents on one stem of 160 symbols, scattered over the docIDs (a long prefix completes to several documents)
    families = []
    for f in range(3):
        stem = text(rnd, 160, letters).replace(b" ", b"a", 1)
        ids = sorted(rnd.choice(n_docs, size=10, replace=False).tolist())
        for i in ids:
            docs[i] = stem + text(rnd, rnd.randint(10, 61), letters)
        families.append(ids)
    long_docs = [i for i, d in enumerate(docs) if len(d) >= 200]
    long_q = [text(rnd, n, letters) for n in rnd.randint(150, 401, size=40)]
    foreign = [docs[i][:int(rnd.randint(150, 201))] + b"z" for i in rnd.choice(long_docs, size=12, replace=False).tolist()]
    short = [docs[i][:int(rnd.randint(5, 61))] for i in rnd.choice(n_docs, size=50, replace=False).tolist()]
    short += [d for d in docs if len(d) <= 60][:25]
    short += [text(rnd, n, letters) for n in rnd.randint(0, 100, size=25)]
    diluted = [diluted_query(docs, *t) for t in DILUTED]
    # (rows of the diluted queries are mostly not full: enough further texts that nine long rows in ten still are)
    more = np.random.RandomState(seed + 1)
    long_q += [text(more, n, letters) for n in more.randint(150, 401, size=45)]
    queries, _ = interleave(rnd, long_q + foreign + diluted, short)
    flag_queries = [text(rnd, n, letters) for n in rnd.randint(150, 2001, size=200)]
    # paging: diluted queries of 1 ... 507 candidates (a text over "abcd " has 15 000 and more: 5 000 launches at three a page)
    paging = [diluted[i] for i in (1, 2, 0, 3, 7, 12)]
    prefixes = [docs[families[0][2]][:150], docs[families[1][0]][:160], docs[long_docs[9]][:170], docs[long_docs[40]][:145]]
    return dict(docs=docs, queries=queries, flag_queries=flag_queries, paging=paging, prefixes=prefixes, families=families, diluted=diluted)


def diluted_query(docs, doc, length, foreign):
    r = np.random.RandomState((1000003 * doc + 1009 * length + foreign) % (2 ** 31))
    q = docs[doc][:length] + text(r, foreign, FOREIGN)
    return q + b"z" * max(0, 150 - len(q))


def table_dictionary(n_docs=3000, seed=13):
    """A dictionary over "abc": 27 trigrams and the wrap's, so a long query has at most 40 n-grams and a table of a_max = 40
    answers it.  -> dict: docs, queries, over (position of the one query with more than 40 n-grams)"""
    rnd = np.random.RandomState(seed)
    docs = [text(rnd, n, b"abc") for n in rnd.randint(3, 120, size=n_docs)]
    long_q = [text(rnd, n, b"abc") for n in rnd.randint(150, 500, size=12)]
    long_q += [docs[i] + docs[i + 1] + docs[i + 2] + docs[i + 3] for i in range(0, 40, 10)]
    short = [docs[i][:20] for i in range(100, 130)] + [text(rnd, n, b"abc") for n in rnd.randint(0, 40, size=10)]
    over = text(rnd, 170, b"abc") + text(rnd, 60, b"abcdefgh")
    queries, at = interleave(rnd, long_q + [over], short)
    return dict(docs=docs, queries=queries, over=at[-1])


def thread_batch(d, seed=17):
    """12 long and 200 short queries over the dense dictionary"""
    rnd = np.random.RandomState(seed)
    docs = d["docs"]
    long_q = [text(rnd, n, b"abcd ") for n in rnd.randint(150, 301, size=8)] + [q for q in d["queries"] if q.endswith(b"z")][:4]
    short = [docs[i][:int(rnd.randint(4, 50))] for i in rnd.choice(len(docs), size=200, replace=False).tolist()]
    return interleave(rnd, long_q, short)[0]


# ---- 2. the limits -------------------------------------------------------------------------------------------------------
A36 = b"abcdefghijklmnopqrstuvwxyz0123456789"
CYR = "абвгдежз" + "abc"

LIMIT_CASES = {
    # name: q, wrap, pad, alphabet of the description, letters of the texts, bytes answered, bytes flagged (None: no such row)
    "q3_12": dict(q=3, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"), letters=b"abcdefghijkl", answered=65536, flagged=65537, doc_65536=True),
    "q2_36": dict(q=2, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"), letters=A36, answered=65535, flagged=65536),
    "q1_36": dict(q=1, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"), letters=A36, answered=65534, flagged=65535),
    "q5_abc": dict(q=5, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"), letters=b"abc", answered=65536, flagged=None),
    "q8_ab": dict(q=8, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"), letters=b"ab", answered=65536, flagged=None),
    "q3_cyr": dict(q=3, wrap=("$", "$"), pad="$", alphabet=("russian", "english", "$"), letters=CYR, answered=65536, flagged=None, doc_65536=True),
    "q3_nowrap": dict(q=3, wrap=("", ""), pad="", alphabet=("english", "numbers", "$"), letters=b"abc", answered=None, flagged=None),
}


def limit_desc(case):
    c = LIMIT_CASES[case]
    return dict(ngram_size=c["q"], wrap=c["wrap"], pad=c["pad"], alphabet=c["alphabet"])


def sized(rnd, n_bytes, letters, head=b""):
    """`head` followed by random symbols, exactly n_bytes long (two-byte letters: the last symbols are one-byte ones)"""
    if isinstance(letters, bytes):
        return (head + text(rnd, max(0, n_bytes - len(head)), letters))[:n_bytes]
    out = head + text(rnd, (n_bytes - len(head)) // 2 + 8, letters)
    cut = out[:n_bytes].decode("utf-8", "ignore").encode("utf-8")             # (a cut inside a letter drops it)
    return cut + b"a" * (n_bytes - len(cut))


def of_windows(rnd, case, w, letters):
    """a text without spaces of exactly w n-gram windows under the case's description"""
    c = LIMIT_CASES[case]
    n_runes = w + c["q"] - 1 - len(c["wrap"][0]) - len(c["wrap"][1])
    return text(rnd, n_runes, letters)


def limits(case, seed=23):
    """-> dict: docs, queries, answered (position of the query at the limit, None in the empty-wrap case), flagged (position of
    the one past it, or None), on_document (positions of answered queries that contain a long dictionary document),
    expect_windows {position: windows}, spaces (empty-wrap case: {position: expected count or None})"""
    c = LIMIT_CASES[case]
    rnd = np.random.RandomState(seed + sorted(LIMIT_CASES).index(case))
    letters = c["letters"]
    docs = [text(rnd, n, letters) for n in rnd.randint(2, 40, size=2000)]
    docs[0] = text(rnd, 30, letters)                           # (the first document must have tokens: indexer_writer.go:70)
    long_at = [150, 700, 1100, 1500, 1900]
    # (symbols; the two-byte letters stay below the 65 536 bytes a document of the device builder may have)
    for at, n in zip(long_at, (300, 2000, 9000, 30000, 60000) if isinstance(letters, bytes) else (300, 2000, 9000, 20000, 36000)):
        docs[at] = text(rnd, n, letters)
    if c.get("doc_65536"):
        docs[1950] = sized(rnd, LONG_MAX, letters)
        long_at.append(1950)
    desc = limit_desc(case)
    queries, expect, on_document, spaces = [], {}, [], {}

    def add(q, w=None, on_doc=False):
        if w is not None:
            expect[len(queries)] = w
        if on_doc:
            on_document.append(len(queries))
        queries.append(q)
        return len(queries) - 1

    answered = flagged = None
    add(docs[3])
    for k in (8, 12, 15):                                       # the steps of `while (H < 2u * G)`
        for w in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            add(of_windows(rnd, case, w, letters), w)
    add(docs[7].decode("utf-8")[:-1].encode("utf-8"))
    add(docs[long_at[1]] + text(rnd, 500, letters), on_doc=True)          # one long document followed by random text
    add(docs[long_at[0]] * 3, on_doc=True)                                 # one long document repeated three times
    if c["answered"] is not None:
        n_wrap = len(c["wrap"][0]) + len(c["wrap"][1])
        if c.get("doc_65536"):
            big = docs[1950]
        else:
            big = sized(rnd, c["answered"], letters, head=docs[long_at[4]])
        assert len(big) == c["answered"]
        answered = add(big, runes_of(big) + n_wrap - c["q"] + 1, on_doc=True)
        if c["flagged"] is not None:
            over = sized(rnd, c["flagged"], letters, head=big)
            flagged = add(over, runes_of(over) + n_wrap - c["q"] + 1)
        add(docs[long_at[2]], on_doc=True)                                 # an answered one behind the flagged one
    else:
        body = text(rnd, 200, letters)
        for q, want in ((b" " * 300 + b"abc" + b" " * 300, None), (b" " * 300 + b"ab" + b" " * 300, 0), (b" " * LONG_MAX, 0),
                        (b" " * 400 + body + b" " * 77, None)):
            spaces[add(q)] = want
        add(docs[long_at[2]], on_doc=True)
    add(docs[11])
    add(b"")
    return dict(docs=docs, desc=desc, queries=queries, answered=answered, flagged=flagged, on_document=on_document,
                expect_windows=expect, spaces=spaces, long_docs=long_at)
