"""LanguageModel.ScoreSentence / ScoreWordIDs for batches on the GPU (lm_score.inc: sg_lm_score_text_batch, _device,
sg_lm_score_word_ids_batch) against the host's one-sentence scorer (sg_lm_score_word_ids, lm.cpp), which restates
pkg/lm/language_model.go:72-92 and ngram_model.go:44-62,163-175.  Device log() and glibc log() are not known to agree to
the bit: scores are compared within 1e-12 relative unless a case says exact."""
import itertools
import os
import sys
import threading

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

LM_DIR = os.path.join(GOLDEN, "lm")
UNK = 0xFFFFFFFF


def _host_ids(lm, ids):
    from suggest_amd import _lib
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    return float(_lib.lib().sg_lm_score_word_ids(lm._h, a.ctypes.data if a.size else None, len(a)))


def _assert_close(dev, host, what=""):
    dev, host = np.asarray(dev, dtype=np.float64), np.asarray(host, dtype=np.float64)
    with np.errstate(invalid="ignore"):                     # (inf - inf: equal infinities pass on the first test)
        ok = (dev == host) | (np.abs(dev - host) <= 1e-12 * np.maximum(1.0, np.abs(host)))
    bad = np.nonzero(~ok)[0]
    assert not len(bad), (what, bad[:10], dev[bad[:10]], host[bad[:10]])


def _offs(lists):
    o = np.zeros(len(lists) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    return o


def _score_ids(lm, lists):
    ids = np.array([w for s in lists for w in s], dtype=np.uint32)
    return lm.score_word_ids_batch(ids, _offs(lists))


@pytest.fixture(scope="module")
def g(reference_tests):
    return reference_tests["lm"]


def test_reference_goldens_through_both_paths(g):
    from suggest_amd import LanguageModel
    lm = LanguageModel(LM_DIR, g["order"], g["startSymbol"], g["endSymbol"])
    sentences = [w for w, _ in g["score_sentence"]]
    expected = np.array([e for _, e in g["score_sentence"]])
    tol = g["tolerance"]
    assert (np.abs(lm.ScoreSentenceBatch(sentences) - expected) < tol).all()
    s, w, u = lm.score_text_batch([" ".join(x) for x in sentences])
    assert (np.abs(s - expected) < tol).all()
    assert list(w) == [len(x) for x in sentences]
    assert list(u) == [sum(lm.GetWordID(t) == UNK for t in x) for x in sentences] and u.any()


@pytest.mark.parametrize("order", [1, 2, 3])
def test_fixture_model_every_short_sentence(order):
    from suggest_amd import LanguageModel
    lm = LanguageModel(LM_DIR, order)
    V = len(lm)
    vocab = list(range(V)) + [UNK]
    lists = [list(c) for n in range(5) for c in itertools.product(vocab, repeat=n)]
    rnd = np.random.RandomState(order)
    lists += [list(rnd.randint(V, V + 4, size=n)) for n in range(1, 6) for _ in range(20)]            # at and past the vocabulary
    lists += [list(rnd.choice([0, 1, V, UNK, 0xFFFFFFFD, 0xFFFFFFFE], size=n)) for n in range(1, 8) for _ in range(20)]
    dev = _score_ids(lm, lists)
    host = np.array([_host_ids(lm, s) for s in lists])
    _assert_close(dev, host, "order %d" % order)
    empty = np.array([len(s) + 2 < order for s in lists])
    assert (dev[empty] == 0.0).all() and (np.signbit(dev[empty]) == False).all()   # no window: exactly +0.0
    unknown_only = np.array([len(s) > 0 and all(w == UNK for w in s) for s in lists])
    _assert_close(dev[unknown_only], host[unknown_only], "unknown words")
    # the token path gives the same rows
    words = [b"dont" if w == UNK else lm.word(w) for w in vocab]
    lines = [b" ".join(words[vocab.index(w)] for w in s) for s in lists if all(w in vocab for w in s)]
    s_txt, w_txt, u_txt = lm.score_text_batch(lines)
    host_txt = np.array([lm.ScoreSentence(lm.Tokenize(x)) for x in lines])
    _assert_close(s_txt, host_txt, "text order %d" % order)
    assert list(w_txt) == [len(lm.Tokenize(x)) for x in lines]


def _write(d, grams):
    for k, lines in grams.items():
        with open(os.path.join(d, "%d-gm" % k), "w") as f:
            f.write("".join("%s\t%d\n" % kv for kv in lines))


def test_orphans_and_a_sparse_unigram_level(tmp_path):
    """an orphan (an n-gram whose prefix is missing from the level below) makes the host divide by a zero count: +Inf, on the
    device too; a 1-gm that repeats a word leaves a hole in the unigram ids, so that level is searched, not indexed"""
    from suggest_amd import LanguageModel
    d = str(tmp_path)
    _write(d, {1: [("<S>", 2), ("a", 3), ("b", 2), ("a", 1), ("</S>", 2)],
               2: [("<S> a", 1), ("a b", 2), ("zz b", 1), ("zz a", 4), ("b </S>", 1)],
               3: [("<S> a b", 1), ("zz b </S>", 1), ("a b </S>", 2)]})
    for order in (1, 2, 3):
        lm = LanguageModel(d, order)
        V = len(lm)
        vocab = list(range(V)) + [UNK, V + 3]
        lists = [list(c) for n in range(5) for c in itertools.product(vocab, repeat=n)]
        dev = _score_ids(lm, lists)
        host = np.array([_host_ids(lm, s) for s in lists])
        _assert_close(dev, host, "order %d" % order)
        if order >= 2:
            assert np.isinf(host).any() and (np.isinf(dev) == np.isinf(host)).all()


def _tok_check(lm, lines):
    s, w, u = lm.score_text_batch(lines)
    vocab = lm._vocab()
    toks = [lm.Tokenize(x) for x in lines]
    assert list(w) == [len(t) for t in toks]
    assert list(u) == [sum(1 for x in t if x not in vocab) for t in toks]
    _assert_close(s, np.array([lm.ScoreSentence(t) for t in toks]), "text")
    return s, w, u


def test_text_path_lines():
    from suggest_amd import LanguageModel
    lm = LanguageModel(LM_DIR, 3, alphabet=("english", "russian", "numbers", "-."))
    rnd = np.random.RandomState(5)
    words = [w.decode() for w in lm.words()] + ["dont", "ёжик"]
    long_line = lambda n: " ".join(words[i] for i in rnd.randint(0, len(words), size=n))
    lines = ["I AM SAM", "ЁЖИК В ТУМАНЕ", "İstanbul'da i am", "   i am sam   ", "...,,,!!!", "", " ", "i \xff am", b"sam \xc3 i \xe2\x82 am \xf0",
             b"\xff\xfe", "Sam-I-am. i.am", "KELVIN K sam", long_line(300), long_line(300).upper(), long_line(100_000)]
    lines = [x.encode("utf-8") if isinstance(x, str) else x for x in lines]
    s, w, u = _tok_check(lm, lines)
    assert w[5] == 0 and s[5] == 0.0 and w[-1] == 100_000


def _cfg5(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_lm
    from suggest_amd.spell import LanguageModel
    tokens = int(os.environ.get("SG_TEST_LM_TOKENS", 50_000_000))
    d = str(tmp_path_factory.mktemp("lm50m"))
    info = make_synthetic_lm.make(d, tokens=tokens, vocab=1_000_000 if tokens >= 20_000_000 else max(1000, tokens // 40), verbose=False)
    lm = LanguageModel(binary=os.path.join(d, "synth.lm"), dictionary=os.path.join(d, "synth.cdb"))
    return info, lm


def _cfg5_sentences(info, n, seed):
    """n sentences cut from the corpus sample: 6 .. 21 words mostly, some above 64, some with an unknown word"""
    T, words = info["corpus_sample"], info["word_list"]
    markers = {info["start_id"], info["end_id"]}
    rnd = np.random.Generator(np.random.PCG64(seed))
    out = []
    while len(out) < n:
        ln = int(rnd.integers(90, 300)) if len(out) % 97 == 0 else int(rnd.integers(0, 22))
        p = int(rnd.integers(0, len(T) - ln))
        ids = [int(x) for x in T[p:p + ln] if int(x) not in markers]
        toks = [words[i] for i in ids]
        if len(out) % 13 == 5 and toks:
            toks[int(rnd.integers(0, len(toks)))] = b"qqzzunknownqq"
        out.append(b" ".join(toks))
    return out


def test_cfg5_scale(tmp_path_factory):
    info, lm = _cfg5(tmp_path_factory)
    lines = _cfg5_sentences(info, 65536, seed=11)
    s, w, u = lm.score_text_batch(lines)
    toks = [x.split() for x in lines]
    assert list(w) == [len(t) for t in toks]
    assert list(u) == [t.count(b"qqzzunknownqq") for t in toks]
    assert (w > 64).sum() >= 600 and (u > 0).sum() > 4000
    host = np.array([lm.ScoreSentence(t) for t in toks])
    _assert_close(s, host, "cfg5 text")
    _assert_close(lm.ScoreSentenceBatch(toks), host, "cfg5 ids")


def test_device_variant_on_a_side_stream_equals_host_buffers():
    import torch
    from suggest_amd import LanguageModel
    from suggest_amd.index import pack_strings
    lm = LanguageModel(LM_DIR, 3)
    rnd = np.random.RandomState(9)
    words = [w.decode() for w in lm.words()] + ["dont", "İ", "Sam,"]
    lines = [" ".join(words[i] for i in rnd.randint(0, len(words), size=rnd.randint(0, 40))) for _ in range(5000)]
    s, w, u = lm.score_text_batch(lines)
    blob, offs = pack_strings(lines)
    d_blob = torch.from_numpy(blob).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_s = torch.zeros(len(lines), dtype=torch.float64, device="cuda")
    d_w = torch.zeros(len(lines), dtype=torch.int32, device="cuda")
    d_u = torch.zeros(len(lines), dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        lm.score_text_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), len(lines), len(blob), d_s.data_ptr(), d_w.data_ptr(), d_u.data_ptr(),
                                   stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d_s.cpu().numpy().view(np.uint64), s.view(np.uint64))
    assert np.array_equal(d_w.cpu().numpy().view(np.uint32), w) and np.array_equal(d_u.cpu().numpy().view(np.uint32), u)
    d_s.zero_()
    lm.score_text_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), len(lines), len(blob), d_s.data_ptr(), None, None,
                               stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d_s.cpu().numpy().view(np.uint64), s.view(np.uint64))


def test_large_batch_takes_the_unstaged_branch():
    from suggest_amd import LanguageModel
    lm = LanguageModel(LM_DIR, 3)
    rnd = np.random.RandomState(13)
    words = [w.decode() for w in lm.words()] + ["dont", "Sam."]
    base = [" ".join(words[i] for i in rnd.randint(0, len(words), size=rnd.randint(0, 60))) for _ in range(4000)]
    lines = [base[i] for i in rnd.randint(0, len(base), size=500_000)]
    lines[::1000] = [("i am sam " * 2000) for _ in lines[::1000]]
    assert sum(len(x) for x in lines) > (64 << 20)
    s, w, u = lm.score_text_batch(lines)
    parts = [lm.score_text_batch(lines[i:i + 25_000]) for i in range(0, len(lines), 25_000)]
    assert np.array_equal(s.view(np.uint64), np.concatenate([p[0] for p in parts]).view(np.uint64))
    assert np.array_equal(w, np.concatenate([p[1] for p in parts])) and np.array_equal(u, np.concatenate([p[2] for p in parts]))


def test_poisoned_scratch_and_rows_change_nothing():
    from suggest_amd import LanguageModel, _lib
    lm = LanguageModel(LM_DIR, 3)
    rnd = np.random.RandomState(17)
    words = [w.decode() for w in lm.words()] + ["dont"]
    lines = [" ".join(words[i] for i in rnd.randint(0, len(words), size=rnd.randint(0, 30))) for _ in range(3000)]
    lists = [list(rnd.randint(0, len(words) + 2, size=rnd.randint(0, 30))) for _ in range(3000)]
    ref = lm.score_text_batch(lines), _score_ids(lm, lists)
    for family in (1, 2):
        with _lib.poisoned(family):
            got = lm.score_text_batch(lines), _score_ids(lm, lists)
            assert _lib.poison_stats()["out_scores"] > 0
        for a, b in zip(ref[0], got[0]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert np.array_equal(ref[1].view(np.uint64), got[1].view(np.uint64))


def test_a_slice_of_an_id_array_and_scores_alone():
    """score_word_ids on sentences 2..4 of a five-sentence id array, handed over as offsets whose first is not zero, equals rows
    2..4 of the whole call bit for bit; score_text without `words` / `unknown` asked for gives the scores of the full call."""
    from suggest_amd import LanguageModel, _lib
    from suggest_amd.index import pack_strings
    lm = LanguageModel(LM_DIR, 3)
    V = len(lm)
    lists = [[0, 1, 2], [UNK], [1, 1, 0, 2, V + 1, 0], [], [2, 0, 1, 1]]
    ids = np.array([w for s in lists for w in s], dtype=np.uint32)
    offs = _offs(lists)
    whole = lm.score_word_ids_batch(ids, offs)
    assert offs[2] != 0
    part = lm.score_word_ids_batch(ids, offs[2:5 + 1])
    assert np.array_equal(part.view(np.uint64), whole[2:5].view(np.uint64))
    _assert_close(whole, np.array([_host_ids(lm, s) for s in lists]))
    lines = [b"i am sam", b"", b"sam i am dont", b"I AM", b"qqzz sam"]
    blob, o = pack_strings(lines)
    blob, o = np.ascontiguousarray(blob, dtype=np.uint8), np.ascontiguousarray(o, dtype=np.uint64)
    full = lm.score_text_batch(lines)
    for want_words, want_unknown in ((False, False), (True, False), (False, True)):
        s, w, u = np.full(len(lines), 7.0), np.full(len(lines), 7, dtype=np.uint32), np.full(len(lines), 7, dtype=np.uint32)
        _lib.check(_lib.lib().sg_lm_score_text_batch(lm._h, 0, blob.ctypes.data, o.ctypes.data, len(lines), s.ctypes.data,
                                                     w.ctypes.data if want_words else None, u.ctypes.data if want_unknown else None))
        assert np.array_equal(s.view(np.uint64), full[0].view(np.uint64))
        assert np.array_equal(w, full[1]) if want_words else np.all(w == 7)
        assert np.array_equal(u, full[2]) if want_unknown else np.all(u == 7)


def test_a_slice_of_an_id_array_above_the_staging_limit():
    """17 M ids (68 MB, above the 64 MiB a synchronous call stages) behind three ids of another sentence, handed over with offsets
    whose first is 3: served, and bit for bit the call on the same ids with offsets from zero."""
    from suggest_amd import LanguageModel
    lm = LanguageModel(LM_DIR, 3)
    n, per = 1_000_000, 17
    ids = np.random.RandomState(23).randint(0, len(lm) + 2, size=3 + n * per).astype(np.uint32)
    offs = 3 + per * np.arange(n + 1, dtype=np.uint64)
    assert n * per * 4 > 64 << 20
    part = lm.score_word_ids_batch(ids, offs)
    whole = lm.score_word_ids_batch(ids[3:], offs - np.uint64(3))
    assert np.array_equal(part.view(np.uint64), whole.view(np.uint64))
    _assert_close(part[:50], np.array([_host_ids(lm, ids[3 + i * per:3 + (i + 1) * per]) for i in range(50)]))


def test_interleaved_with_predict_and_threads():
    from suggest_amd import LanguageModel, SpellChecker
    lm = LanguageModel(LM_DIR, 3)
    rnd = np.random.RandomState(21)
    words = [w.decode() for w in lm.words()] + ["dont"]
    lines = [" ".join(words[i] for i in rnd.randint(0, len(words), size=rnd.randint(0, 25))) for _ in range(2000)]
    alone = lm.score_text_batch(lines)
    sc = SpellChecker(lm, device=0)
    queries = ["i am sa", "sam i", "i do not li", "green eg", "am", ""] * 50
    p0 = sc.predict_batch(queries, 3, 0.5)
    mid = lm.score_text_batch(lines)
    p1 = sc.predict_batch(queries, 3, 0.5)
    for a, b in zip(alone, mid):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(p0[1], p1[1])
    valid = np.arange(p0[0].shape[1])[None, :] < np.minimum(p0[1], p0[0].shape[1])[:, None]
    assert np.array_equal(p0[0][valid], p1[0][valid])
    results, errors = [None] * 4, []

    def worker(k):
        try:
            results[k] = [lm.score_text_batch(lines) for _ in range(3)]
        except Exception as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for rs in results:
        for r in rs:
            for a, b in zip(alone, r):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
