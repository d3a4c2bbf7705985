"""Shared by tests/test_predict_shapes_cpu.py and tests/test_gpu_predict_topk.py: a crafted order-3 language model whose
vocabulary, continuation lists and queries put SpellChecker.Predict on every path it has above topK = 20 — completion lists
below, at and above topK, merged candidate lists above topK (rows of topK + 1 entries) and above a wavefront, continuation
lists on both sides of 64 entries, counts drawn from {1, 2, 3} (ties everywhere: the stable order shows), last words above
the wavefront kernel's 128 n-grams.  Everything is seeded; the yardstick is the CPU oracle (oracle/spell_oracle.inc), and
conditions() says — from the oracle and the construction alone — how many queries of every kind a batch holds."""
import os

import numpy as np

import oracle
from test_spell import SPELL_INDEX

ALPHA = ("english", "numbers")
ORDER = 3
START, END = "<S>", "</S>"
LETTERS = "abcdefghijklmnopqrstuvwxyz"
SYMBOLS = LETTERS + "0123456789"
SPECIAL = 0xFFFFFFF0                      # counts at and above: SG_COUNT_TOO_LONG and friends (no row)

GROUP_SIZES = (31, 32, 33, 63, 64, 65, 66, 100, 129, 300, 1100)
# (3-letter prefixes of the groups; the family bases differ from one another, and from every prefix, in at least two positions)
GROUP_PREFIXES = ("bda", "cfe", "dgi", "fho", "gju", "hka", "jle", "kmi", "lno", "mpu", "nra")
FAMILY_BASES = ("tovu", "sewy", "rixa", "qazo")
FAMILY_COMPLETIONS = (20, 40, 70, 1000)
LIST_LENGTHS = (0, 1, 63, 64, 65, 66, 128, 129, 1000)
UNKNOWN = "zzunknown"                     # not a word of the model
# what tests/test_gpu_predict_topk.py asks the device for; tests/test_predict_shapes_cpu.py holds conditions() to every pair
LARGE_TOP_KS = (32, 33, 63, 64, 65, 100, 128, 1023)
SIMILARITIES = (0.3, 0.2)
GPU_CASES = tuple((k, s) for k in LARGE_TOP_KS for s in SIMILARITIES) + ((5, 0.3),)


def _distinct(rnd, n, length, alphabet, taken):
    out = []
    while len(out) < n:
        w = "".join(alphabet[int(i)] for i in rnd.randint(0, len(alphabet), size=length))
        if w not in taken:
            taken.add(w)
            out.append(w)
    return out


def _spread(rnd, pools, n):
    """n distinct words, taken in turn from every pool (each in a random order) until n are there"""
    pools = [[p[int(i)] for i in rnd.permutation(len(p))] for p in pools]
    out, depth = [], 0
    while len(out) < n:
        took = False
        for p in pools:
            if depth < len(p) and len(out) < n:
                out.append(p[depth])
                took = True
        assert took, "the pools hold fewer than %d words" % n
        depth += 1
    return out


def build(directory, seed=17, big_group=1100, big_family=1000):
    """writes <directory>/{1,2,3}-gm -> the model's pieces (a dict).  big_group / big_family: the sizes of the largest prefix
    group and the largest family (smaller for a batch that must stay quick; the other sizes are what the topK values need)."""
    rnd = np.random.RandomState(seed)
    m = dict(directory=directory, groups=[], families=[])
    pools = []
    for size, prefix in zip(GROUP_SIZES[:-1] + (big_group,), GROUP_PREFIXES):
        words = [prefix + s for s in _distinct(rnd, size, 3, LETTERS, set())]
        m["groups"].append(dict(prefix=prefix, size=size, words=words))
        pools.append(words)
    for base, n_comp in zip(FAMILY_BASES, FAMILY_COMPLETIONS[:-1] + (big_family,)):
        # (16 random letters behind the base: ~20 distinct n-grams, so that the base's neighbours out-score the completions)
        comps = [base + s for s in _distinct(rnd, n_comp, 16, LETTERS, set())]
        neigh = [base[:p] + c + base[p + 1:] for p in range(4) for c in SYMBOLS if c != base[p]]
        m["families"].append(dict(base=base, completions=comps, neighbours=neigh))
        pools += [comps, neigh]
    for i, a in enumerate(FAMILY_BASES):
        for b in FAMILY_BASES[i + 1:] + GROUP_PREFIXES:
            assert sum(x != y for x, y in zip(a, b)) >= 2, (a, b)
    stem = "".join(LETTERS[int(i)] for i in rnd.randint(0, 26, size=140))
    taken = set()
    long_stem = [stem + _distinct(rnd, 1, int(rnd.randint(5, 301)), LETTERS, taken)[0] for _ in range(90)]   # 145 .. 440 letters
    long_other = [_distinct(rnd, 1, int(rnd.randint(130, 501)), LETTERS, taken)[0] for _ in range(30)]
    m["stem"], m["long_stem"], m["long_other"] = stem, long_stem, long_other
    # ---- contexts: a word per list length, two pairs of words (trigram contexts), a word with a list of long words ----
    ctx_word = {n: "cx%d" % n for n in LIST_LENGTHS}
    pairs = {64: ("cxa", "cxb"), 65: ("cxc", "cxd")}
    lists = {}                                                   # the scorer's key (two words) -> {word: count}

    def counted(words):
        return {w: int(c) for w, c in zip(words, rnd.randint(1, 4, size=len(words)))}

    for n in LIST_LENGTHS[1:]:
        lists[(START, ctx_word[n])] = counted(_spread(rnd, pools, n))
    for n, pair in pairs.items():
        lists[pair] = counted(_spread(rnd, pools, n))
    half = [long_stem[i] for i in range(0, 90, 2)] + [long_other[i] for i in range(0, 30, 2)]
    lists[(START, "cxlong")] = counted(half + _spread(rnd, pools, 40))
    m["lists"], m["ctx_word"], m["pairs"] = lists, ctx_word, pairs
    m["contexts"] = [""] + [ctx_word[n] + " " for n in LIST_LENGTHS] + ["%s %s " % p for p in pairs.values()] + ["cxlong ", UNKNOWN + " "]
    # ---- the vocabulary: de-duplicated, shuffled (word id = line number of 1-gm; ties break by id) ----
    vocab = [w for p in pools for w in p] + long_stem + long_other + list(ctx_word.values()) + [w for p in pairs.values() for w in p] + ["cxlong", START, END]
    vocab = sorted(set(vocab))
    assert UNKNOWN not in vocab
    vocab = [vocab[int(i)] for i in rnd.permutation(len(vocab))]
    m["vocab"] = vocab
    for g in m["groups"]:                                         # a group's prefix completes to the group and to nothing else
        assert sum(w.startswith(g["prefix"]) for w in vocab) == g["size"], g["prefix"]
    for f in m["families"]:
        assert f["base"] not in vocab and sum(w.startswith(f["base"]) for w in vocab) == len(f["completions"])
    with open(os.path.join(directory, "1-gm"), "w") as f:
        f.write("".join("%s\t%d\n" % (w, 1 + int(c)) for w, c in zip(vocab, rnd.randint(0, 50, size=len(vocab)))))
    with open(os.path.join(directory, "2-gm"), "w") as f:
        for (a, b), cont in lists.items():
            f.write("%s %s\t%d\n" % (a, b, sum(cont.values())))
            if a == START:
                f.write("".join("%s %s\t%d\n" % (b, w, c) for w, c in cont.items()))
    with open(os.path.join(directory, "3-gm"), "w") as f:
        for (a, b), cont in lists.items():
            f.write("".join("%s %s %s\t%d\n" % (a, b, w, c) for w, c in cont.items()))
    return m


def open_oracle(m):
    """-> (OracleLM, OracleIndex) of the files build() wrote"""
    lm = oracle.OracleLM(m["directory"], ORDER, alphabet=ALPHA)
    assert [w.decode() for w in lm.words()] == m["vocab"]
    return lm, oracle.OracleIndex(lm.words(), **SPELL_INDEX)


def _cut_at(ix, text, n_grams):
    """the shortest prefix of `text` with n_grams n-grams, as the index tokenises a query"""
    for n in range(1, len(text) + 1):
        if len(ix.tokenize(text[:n])) == n_grams:
            return text[:n]
    raise AssertionError("no prefix of %d n-grams" % n_grams)


def last_words(m, ix):
    """the last words of the crafted batch, in kinds: [(kind, word)]"""
    rnd = np.random.RandomState(23)
    vocab = set(m["vocab"])
    out = []
    for g in m["groups"]:
        p = g["prefix"]
        typo = p[0] + "7" + p[2]
        assert not any(w.startswith(typo) for w in vocab)
        out += [("prefix", p), ("prefix+1", g["words"][int(rnd.randint(0, g["size"]))][:4]), ("typo", typo)]
    for f in m["families"]:
        b = f["base"]
        out += [("base", b), ("base-1", b[:3]), ("base+1", f["completions"][int(rnd.randint(0, len(f["completions"])))][:5])]
    stem = m["stem"]
    mid = len(stem) // 2
    broken = stem[:mid] + "7" + stem[mid + 1:]                   # (no long word holds a digit: no completion, whatever the letters around it)
    assert not any(w.startswith(broken) for w in vocab)
    out += [("long128", _cut_at(ix, stem, 128)), ("long129", _cut_at(ix, stem, 129)), ("stem", stem), ("stem typo", broken)]
    return out


def queries(m, ix=None):
    """the crafted batch (bytes): every context x every last word, then a few variants a keyboard produces"""
    if "queries" not in m:
        ix = ix or open_oracle(m)[1]
        words = [w for _, w in last_words(m, ix)]
        qs = [(c + w).encode() for c in m["contexts"] for w in words]
        c63, c65 = m["ctx_word"][63], m["ctx_word"][65]
        g, f = m["groups"][7], m["families"][1]
        qs += [("%s %s" % (c63, g["prefix"])).upper().encode(), ("%s  %s" % (c65, f["base"])).encode(), ("  %s   %s  " % m["pairs"][64] + g["prefix"]).encode(),
               ("%s %s" % (c65.upper(), f["base"][:3])).encode(), ("%s, %s" % (c63, m["stem"].upper())).encode(), b"", b" ,. -", b"   "]
        m["queries"] = qs
    return m["queries"]


def scorer_key(tokens):
    """the two words LanguageModel.Next hands to NGramModel.Next at order 3 (language_model.go:100-112), of the tokens in
    front of the last word; None: no context, no scorer"""
    n = len(tokens)
    if n == 0:
        return None
    if n == 1:
        return (START, tokens[0])
    return (tokens[0], tokens[1]) if n <= 3 else (tokens[-2], tokens[-1])


def continuation_counts(m, lm, queries_):
    """-> (list length [n], counts [n][V]: row i = the continuation count of every word id under query i's scorer), from the
    construction (build()'s lists) and the oracle's tokeniser and word ids"""
    word_id = {w: i for i, w in enumerate(m["vocab"])}
    per_key = {}
    for key, cont in m["lists"].items():
        a = np.zeros(len(m["vocab"]), dtype=np.int64)
        for w, c in cont.items():
            a[word_id[w]] = c
        per_key[key] = a
    none = np.zeros(len(m["vocab"]), dtype=np.int64)
    length, rows, last = [], [], []
    for q in queries_:
        toks = [t.decode() for t in lm.tokenize(q)]
        key = scorer_key(toks[:-1])
        length.append(len(m["lists"].get(key, ())))
        rows.append(per_key.get(key, none))
        last.append(toks[-1] if toks else None)
    return np.array(length), rows, last


def conditions(m, lm, ix, top_k, similarity):
    """How many queries of every kind the crafted batch holds at (top_k, similarity): from the oracle and the construction alone."""
    qs = queries(m, ix)
    if "per_query" not in m:
        m["per_query"] = continuation_counts(m, lm, qs)
    length, cont, last = m["per_query"]
    have = np.array([w is not None for w in last])
    wb, wo = oracle.pack_strings([w or "" for w in last])
    ac = ix.autocomplete_batch(wb, wo, top_k + 1)[1]             # (completions of the LAST WORD, one more than top_k asked for)
    ok = have & (ac < SPECIAL)
    n_grams = np.array([len(ix.tokenize(w)) if w else 0 for w in last])
    oi, oc = lm.predict_batch(ix, *oracle.pack_strings(qs), top_k, similarity)
    rows = oc < SPECIAL
    tie_nz = tie_0 = 0
    for i in np.nonzero(rows & (length > 0))[0]:
        c = cont[i][oi[i, :int(oc[i])]]
        tie_0 += int((c == 0).sum() >= 2)
        tie_nz += int(any((c == v).sum() >= 2 for v in (1, 2, 3)))
    return dict(
        queries=len(qs),
        completions_at_least_top_k=int((ok & (ac >= top_k)).sum()), completions_above_top_k=int((ok & (ac > top_k)).sum()),
        completions_below_top_k=int((ok & (ac < top_k)).sum()),
        full_rows=int((rows & (oc == top_k + 1)).sum()),
        rows_above_64=int((rows & (oc > 64)).sum()),
        rows_above_64_list_at_most_64=int((rows & (oc > 64) & (length > 0) & (length <= 64)).sum()),
        rows_above_64_list_above_64=int((rows & (oc > 64) & (length > 64)).sum()),
        ties_nonzero=tie_nz, ties_zero=tie_0,
        long_with_completions=int((ok & (n_grams > 128) & (ac >= 1)).sum()), long_without_completions=int((ok & (n_grams > 128) & (ac == 0)).sum()))


class Replay:
    """stands in for a SpellChecker in test_spell._assert_same_predictions: predict_batch returns the rows it was given"""

    def __init__(self, ids, counts):
        self.ids, self.counts = ids, counts

    def predict_batch(self, blob=None, offs=None, top_k=5, similarity=0.5):
        return self.ids, self.counts
