"""The language model's host side at every order the C ABI takes (1 .. 8), against the oracle: the references the GPU tests of
test_gpu_lm_orders.py lean on (sg_lm_score_word_ids, Tokenize + ScoreSentence, the file-route builders and loaders).  Also the
generators and the hand-written orphan model those tests share."""
import itertools
import os

import numpy as np
import pytest

import oracle

UNK = 0xFFFFFFFF
NO_CONTEXT = 0xFFFFFFFD
ORDERS = (1, 2, 3, 4, 5, 6, 7, 8)
ALPHA = ("english", "numbers")


def _levels(m):
    return [m.level(i) for i in range(int(m.order))]


def assert_same_model(a, b, what):
    """(test_gpu_lm_build._assert_same, restated here so that this module needs nothing a GPU test file holds)"""
    assert int(a.order) == int(b.order), what
    assert list(a.words()) == list(b.words()), what
    for i, ((ac, av, at), (bc, bv, bt)) in enumerate(zip(_levels(a), _levels(b))):
        assert np.array_equal(ac, bc), (what, "containers", i)
        assert np.array_equal(av, bv), (what, "values", i)
        assert at == bt, (what, "total", i)


def make_vocab(stems, endings):
    return [s + e for s in stems for e in endings]


def zipf_corpus(vocab, n_sentences, max_words, seed, families=0):
    """-> list of sentences (lists of words): Zipf-distributed words, 1 .. max_words per sentence.  `families`: that many of
    the sentences come back several times with another last word, so that one long context has several continuations with
    different counts (what a language model re-ranks by)."""
    rnd = np.random.RandomState(seed)
    out = []
    for _ in range(n_sentences):
        n = int(rnd.randint(1, max_words + 1))
        out.append([vocab[int(i)] for i in rnd.zipf(1.3, size=n) % len(vocab)])
    for f in range(families):
        s = out[int(rnd.randint(0, n_sentences))]
        if len(s) < 3:
            continue
        for copies, shift in ((3, 1), (2, 2), (1, 3)):
            alt = s[:-1] + [vocab[(vocab.index(s[-1]) + shift) % len(vocab)]]
            out += [list(alt) for _ in range(copies)]
    return out


def corpus_text(sentences):
    return ("\n".join(" ".join(s) for s in sentences) + "\n").encode()


def host_ids(lm, ids):
    """the product's host scorer of one sentence of ids (sg_lm_score_word_ids, lm.cpp)"""
    from suggest_amd import _lib
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    return float(_lib.lib().sg_lm_score_word_ids(lm._h, a.ctypes.data if a.size else None, len(a)))


def oracle_ids(ora, ids):
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    return float(oracle.lib().or_lm_score_word_ids(ora._h, a.ctypes.data if a.size else None, len(a)))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


# ---- a small generated corpus, both file routes, every order ----
SMALL_VOCAB = make_vocab(["ba", "ca", "mi", "lo"], ["n", "t", "nd", "rk"])


@pytest.fixture(scope="module")
def small_corpus():
    return zipf_corpus(SMALL_VOCAB, 300, 14, seed=2)


@pytest.mark.parametrize("order", ORDERS)
def test_host_product_equals_oracle_on_a_generated_corpus(order, small_corpus, tmp_path):
    from suggest_amd import LanguageModel
    text = corpus_text(small_corpus)
    prod, ora = tmp_path / "prod", tmp_path / "ora"
    prod.mkdir(); ora.mkdir()
    LanguageModel.build_files(text, str(prod), order, "<S>", "</S>", ALPHA, ("\n",))
    oracle.lm_build_files(text, str(ora), order, "<S>", "</S>", ALPHA, ("\n",))
    # "count" numbering does not depend on the order of the files' lines: the two routes are compared whole
    lm = LanguageModel(str(prod), order, "<S>", "</S>", ALPHA, id_order="count")
    om = oracle.OracleLM(str(ora), order, "<S>", "</S>", ALPHA, id_order="count")
    assert_same_model(lm, om, "order %d" % order)
    assert_same_model(lm, oracle.OracleLM(str(prod), order, "<S>", "</S>", ALPHA, id_order="count"), "order %d, product files" % order)
    assert len(lm.level(order - 1)[1]) > (0 if order > 1 else 1)      # the top level holds entries (867 at order 8)
    rnd = np.random.RandomState(100 + order)
    words = SMALL_VOCAB + ["zzunknown", "<S>", "</S>"]
    sentences = [list(s) for s in small_corpus[:150]]
    sentences += [[words[int(i)] for i in rnd.randint(0, len(words), size=int(rnd.randint(0, 15)))] for _ in range(150)]
    for s in small_corpus[150:250]:                                    # a corpus sentence with one word replaced: deep prefixes, then a miss
        s = list(s)
        s[int(rnd.randint(0, len(s)))] = words[int(rnd.randint(0, len(words)))]
        sentences.append(s)
    assert len(sentences) == 400
    assert _same_bits([lm.ScoreSentence(s) for s in sentences], [om.score_sentence(s) for s in sentences])
    assert _same_bits([lm.Score(s[:order]) for s in sentences], [om.score(s[:order]) for s in sentences])
    contexts = []
    for i in range(400):                                               # windows of the corpus (seen), shorter and longer than the order
        s = small_corpus[int(rnd.randint(0, len(small_corpus)))]
        n = int(rnd.randint(0, 12))
        cut = int(rnd.randint(0, len(s) + 1))
        ctx = list(s[max(0, cut - n):cut])
        if i % 5 == 0 and ctx:
            ctx[int(rnd.randint(0, len(ctx)))] = "zzunknown"
        contexts.append(ctx)
    statuses = set()
    for ctx in contexts:
        for model_level in (False, True):
            for w in (SMALL_VOCAB[0], SMALL_VOCAB[5], "zzunknown", "</S>"):
                got, want = lm.next_score(ctx, w, model_level), om.next_score(ctx, w, model_level)
                assert got[0] == want[0] and _same_bits([got[1]], [want[1]]), (ctx, w, model_level, got, want)
                statuses.add(want[0])
    # a scorer, no scorer, the error: all three met (at order 1 every context is an error: none is shorter than the order)
    assert statuses == ({2} if order == 1 else {0, 1, 2})


# ---- a hand-written model with orphans on every level up to the eighth ----
# test_gpu_lm_score.py::test_orphans_and_a_sparse_unigram_level's files, and above them 4- to 8-grams: chains that go on
# from a known 3-gram, entries whose prefix is missing from the level below ("b a b </S>": no 3-gram "b a b"; "zz a b a": zz is
# no word), and entries whose prefix is itself such an orphan ("zz b </S> a" under the orphan "zz b </S>", "b a b </S> a"
# under the orphan 4-gram).  A 1-gm that repeats a word leaves a hole in the unigram ids.
ORPHAN_GRAMS = {
    1: [("<S>", 2), ("a", 3), ("b", 2), ("a", 1), ("</S>", 2)],
    2: [("<S> a", 1), ("a b", 2), ("zz b", 1), ("zz a", 4), ("b </S>", 1), ("b a", 3)],
    3: [("<S> a b", 1), ("zz b </S>", 1), ("a b </S>", 2), ("a b a", 2), ("b b a", 5), ("zz a b", 1)],
    4: [("<S> a b a", 2), ("<S> a b </S>", 1), ("zz b </S> a", 3), ("b a b </S>", 2), ("a b a b", 1), ("zz a b a", 2), ("b b a b", 1)],
    5: [("<S> a b a b", 1), ("b a b </S> a", 4), ("zz b </S> a b", 2), ("a a a a a", 1), ("a b a b </S>", 1), ("zz a b a b", 3)],
    6: [("<S> a b a b </S>", 1), ("b a b </S> a b", 2), ("zz b </S> a b a", 1), ("a a a a a b", 2), ("b b b b b b", 3),
        ("zz a b a b </S>", 1)],
    7: [("<S> a b a b </S> a", 1), ("b a b </S> a b a", 2), ("a a a a a b b", 1), ("zz a b a b </S> b", 2), ("b b a b a b a", 1),
        ("a a a a a a b", 2)],
    8: [("<S> a b a b </S> a b", 2), ("b a b </S> a b a b", 1), ("a a a a a b b a", 3), ("zz zz a b a b a b", 1), ("b b a b a b a a", 1),
        ("a a a a a a b a", 1), ("</S> </S> </S> </S> </S> </S> </S> a", 2)],
}


def write_orphan_model(directory, order=8):
    for k in range(1, order + 1):
        with open(os.path.join(directory, "%d-gm" % k), "w") as f:
            f.write("".join("%s\t%d\n" % kv for kv in ORPHAN_GRAMS[k]))


def orphan_sentences(lm, seed, n=300):
    """sentences of 6 .. 12 ids cut from the model's own n-grams, glued and with a word replaced now and then: the windows of
    orders 7 and 8, which no sentence of five words has"""
    rnd = np.random.RandomState(seed)
    ids = {w: (lm.GetWordID(w) if w != "zz" else UNK) for g in ORPHAN_GRAMS.values() for line, _ in g for w in line.split(" ")}
    grams = [[ids[w] for w in line.split(" ") if w not in ("<S>", "</S>")] for k in (5, 6, 7, 8) for line, _ in ORPHAN_GRAMS[k]]
    out = []
    while len(out) < n:
        s = grams[int(rnd.randint(0, len(grams)))] + grams[int(rnd.randint(0, len(grams)))]
        s = s[int(rnd.randint(0, 3)):][:int(rnd.randint(6, 13))]
        if len(s) < 6:
            continue
        if len(out) % 4 == 0:
            s[int(rnd.randint(0, len(s)))] = [UNK, ids["a"], ids["b"], ids["</S>"]][int(rnd.randint(0, 4))]
        out.append(s)
    return out


@pytest.mark.parametrize("order", ORDERS)
def test_host_product_equals_oracle_on_orphans_up_to_level_eight(order, tmp_path):
    from suggest_amd import LanguageModel
    write_orphan_model(str(tmp_path))
    lm = LanguageModel(str(tmp_path), order)
    om = oracle.OracleLM(str(tmp_path), order)
    assert_same_model(lm, om, "orphans, order %d" % order)
    for k, (c, v, _) in enumerate(_levels(lm)):
        if k:                                                          # no entry is dropped, and every level has a bucket of orphans
            assert len(v) == len(ORPHAN_GRAMS[k + 1]) and int(c[-1] >> np.uint64(32)) == NO_CONTEXT, k
    V = len(lm)
    vocab = list(range(V)) + [UNK]                                     # every word, the hole of the repeated one, an unknown word
    lists = [list(c) for n in range(6) for c in itertools.product(vocab, repeat=n)] + orphan_sentences(lm, order)
    host = np.array([host_ids(lm, s) for s in lists])
    want = np.array([oracle_ids(om, s) for s in lists])
    assert _same_bits(host, want)
    if order >= 2:
        assert np.isinf(want).any()                                    # an orphan's count over the zero count of its missing prefix
    words = [w.decode() for w in lm.words()] + ["zz"]
    rnd = np.random.RandomState(order)
    for ctx in [list(c) for n in range(4) for c in itertools.product(words, repeat=n)] + \
               [[words[int(i)] for i in rnd.randint(0, len(words), size=n)] for n in (4, 5, 6, 7) for _ in range(40)]:
        for model_level in (False, True):
            for w in words:
                got, want1 = lm.next_score(ctx, w, model_level), om.next_score(ctx, w, model_level)
                assert got[0] == want1[0] and _same_bits([got[1]], [want1[1]]), (ctx, w, model_level, got, want1)


# ---- the word tokeniser with U+FFFD and Russian letters in the alphabet ----
TOKENIZE_INPUTS = [
    b"\xff\xfe\xfd",                                                   # bytes that begin nothing: one token of three U+FFFD
    b"ab\xc3", b"\xc3 ab", b"a\xc3b",                                  # a lone lead byte: at the end, alone, inside a word
    b"\xe4\xb8", b"x\xe4\xb8y", b"\xe4",                               # a 3-byte sequence cut after two bytes / one
    b"\xf0\x9f\x98", b"\xf0\x9f", b"\xf0\x9f\x98z", b"\xf0",           # a 4-byte sequence cut after three / two / one
    b"\xed\xa0\x80", b"a\xed\xbf\xbfb",                                # surrogates, encoded
    b"\xc0\xaf", b"\xe0\x80\xaf", b"\xf0\x80\x80\xaf", b"\xc1\xbf",    # overlong forms
    b"\xf4\x90\x80\x80", b"\xf8\x88\x80\x80\x80",                      # above U+10FFFF; a 5-byte form
    b"\x80", b"\xbf\xbf a \x80",                                       # continuation bytes on their own
    "\ufffd real \ufffd\ufffd".encode(),                               # U+FFFD itself, encoded
    "ПРИВЕТ ".encode() + b"\xff " + "МИР".encode() + b"\xfe " + "Привет ёжик ЁЖИК".encode() + b"\xd0",
    "Привет".encode() + b"\xff" + "Мир".encode(),
    b"  \xff  \xfe\xfd  ", b"", b" ", b"\xff" * 40,
]


def test_host_tokenizer_equals_oracle_with_the_replacement_rune_in_the_alphabet():
    from suggest_amd import LanguageModel
    lm_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
    alpha = ("english", "russian", "numbers", "\ufffd")
    lm = LanguageModel(lm_dir, 3, alphabet=alpha)
    ora = oracle.OracleLM(lm_dir, 3, alphabet=alpha)
    assert lm.Tokenize(b"\xff\xfe\xfd") == ["\ufffd\ufffd\ufffd".encode()]                 # one 9-byte token
    assert lm.Tokenize(b"\xff" * 40) == [("\ufffd" * 40).encode()]                          # (three bytes for one: the wrappers' buffers hold it)
    for text in TOKENIZE_INPUTS:
        assert lm.Tokenize(text) == ora.tokenize(text), text
    # U+023A lower-cases to U+2C65: two bytes become three.  U+2C65 goes into the alphabet as a custom symbol
    alpha = ("english", "russian", "numbers", "\ufffdⱥ")
    lm = LanguageModel(lm_dir, 3, alphabet=alpha)
    ora = oracle.OracleLM(lm_dir, 3, alphabet=alpha)
    assert lm.Tokenize("aȺb") == ["aⱥb".encode()]
    for text in TOKENIZE_INPUTS + ["ȺȺȺ".encode(), "xȺ".encode() + b"\xc3", "Ⱥ".encode() * 30, "Ⱥ ⱥȻ".encode()]:
        assert lm.Tokenize(text) == ora.tokenize(text), text
