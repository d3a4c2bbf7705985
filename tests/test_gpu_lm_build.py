"""LanguageModel.from_corpus (sg_lm_build_device): the language model of a corpus built on the GPU.  The yardstick is always the
file route — the oracle's builder and loader (oracle.lm_build_files + oracle.OracleLM) and the product's host builder and loader
(LanguageModel.build_files + LanguageModel(directory)) — never the code under test: levels are compared with np.array_equal on
containers, values and total, words as lists.

Numbering.  id_order "count" does not depend on the order of the lines in the count files, so both file routes are compared
whole.  id_order "lines" numbers the words by the lines of 1-gm: the product's host builder writes them in order of first
appearance (which is what from_corpus restates), the oracle's builder writes them sorted by bytes.  So for "lines" the arrays are
compared with the product's files read by BOTH loaders (the product's and the oracle's), and with the oracle's own files as
n-gram -> count tables spelled in words, which no numbering touches."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

LM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
NO_CONTEXT = 0xFFFFFFFD
ALPHA_WIDE = ("english", "russian", "numbers", "-'")
SEPS_WIDE = (".", "?", "!", "\n")


def _levels(m):
    return [m.level(i) for i in range(int(m.order))]


def _assert_same(a, b, what):
    assert int(a.order) == int(b.order), what
    assert list(a.words()) == list(b.words()), what
    for i, ((ac, av, at), (bc, bv, bt)) in enumerate(zip(_levels(a), _levels(b))):
        assert np.array_equal(ac, bc), (what, "containers", i)
        assert np.array_equal(av, bv), (what, "values", i)
        assert at == bt, (what, "total", i)


def _ngram_table(m):
    """{(word, .., word): count} per level and the totals, decoded from the packed levels: independent of the numbering"""
    words = list(m.words())
    out, prev = [], None
    for c, v, total in _levels(m):
        ctx = np.full(len(v), NO_CONTEXT, dtype=np.uint64)
        starts = (c & np.uint64(0xFFFFFFFF)).astype(np.int64)
        for j in range(len(c)):
            ctx[starts[j]:(starts[j + 1] if j + 1 < len(c) else len(v))] = c[j] >> np.uint64(32)
        grams = []
        for e in range(len(v)):
            w = words[int(v[e] >> np.uint64(32))]
            grams.append((w,) if prev is None else prev[int(ctx[e])] + (w,))
        out.append(({g: int(v[e] & np.uint64(0xFFFFFFFF)) for e, g in enumerate(grams)}, total))
        assert len(out[-1][0]) == len(grams)
        prev = grams
    return out


def _check_against_file_routes(text, order, alpha, seps, tmp_path, tag, start="<S>", end="</S>"):
    """from_corpus(text) against both file routes, both numberings -> the two device-built models"""
    from suggest_amd.spell import LanguageModel
    raw = text.encode() if isinstance(text, str) else bytes(text)
    prod, ora = tmp_path / ("prod_" + tag), tmp_path / ("ora_" + tag)
    prod.mkdir(); ora.mkdir()
    LanguageModel.build_files(raw, str(prod), order, start, end, alpha, seps)
    oracle.lm_build_files(raw, str(ora), order, start, end, alpha, seps)
    built = {}
    for id_order in ("count", "lines"):
        dev = LanguageModel.from_corpus(raw, order, start, end, alpha, seps, id_order=id_order)
        _assert_same(dev, LanguageModel(str(prod), order, start, end, alpha, id_order=id_order), (tag, id_order, "product files"))
        _assert_same(dev, oracle.OracleLM(str(prod), order, start, end, alpha, id_order=id_order), (tag, id_order, "oracle loader, product files"))
        ora_lm = oracle.OracleLM(str(ora), order, start, end, alpha, id_order=id_order)
        if id_order == "count":
            _assert_same(dev, ora_lm, (tag, id_order, "oracle files"))
        else:
            assert _ngram_table(dev) == _ngram_table(ora_lm), (tag, id_order, "oracle files, as n-gram tables")
        built[id_order] = dev
    return built


def _messy_text():
    """the generator of test_spell.py::test_lm_builder_matches_oracle_on_messy_text, restated"""
    rnd = np.random.RandomState(11)
    vocab = ["alpha", "beta", "Gamma", "дельта", "ЭПСИЛОН", "x-ray", "e.g", "42", "naïve", "don't"]
    text = ""
    for _ in range(400):
        text += " ".join(vocab[int(i)] for i in rnd.randint(0, len(vocab), size=int(rnd.randint(0, 9))))
        text += ["\n", ".", "!", " ?", "\n\n", " ", ";"][int(rnd.randint(0, 7))]
    return text.encode() + b"\xff tail \xc3\n"


def test_reference_fixture(reference_tests):
    from suggest_amd.spell import LanguageModel
    from test_lm_binary import _levels_of_file
    g = reference_tests["lm"]
    b = g["build"]
    dev = LanguageModel.from_corpus(b["text"], g["order"], g["startSymbol"], g["endSymbol"], b["alphabet"], b["separators"], id_order="count")
    order, levels = _levels_of_file(os.path.join(LM_DIR, "test.lm"))
    assert dev.order == order
    for i, (c, v, total) in enumerate(levels):
        dc, dv, dt = dev.level(i)
        assert np.array_equal(dc, c) and np.array_equal(dv, v) and dt == total, i
    assert dev.words() == LanguageModel(LM_DIR, id_order="count").words()
    for sent, expected in g["score_sentence"]:
        assert abs(dev.ScoreSentence(sent) - expected) < g["tolerance"], sent


def test_messy_text(tmp_path):
    text = _messy_text()
    for n, (seps, alpha) in enumerate(((SEPS_WIDE, ALPHA_WIDE), (("\n",), ("english", "numbers")))):
        _check_against_file_routes(text, 4, alpha, seps, tmp_path, "messy%d" % n)


def test_messy_text_variants(tmp_path):
    text = _messy_text()
    # a separator of three bytes, next to invalid bytes and to a lead byte of its own kind
    sep = "。".encode()
    wide = text.replace(b"!", sep) + b"\xe3" + sep + b"a\xe3\x80" + sep + b"b " + sep + sep + b" c\x82" + sep[:2]
    _check_against_file_routes(wide, 4, ALPHA_WIDE, ("。", "\n", "?"), tmp_path, "widesep")
    # a separator that is also in the alphabet: it still cuts
    _check_against_file_routes(text, 4, ("english", "russian", "numbers", "-'."), (".", "\n", "a"), tmp_path, "sepalpha")
    # U+FFFD in the alphabet: invalid bytes become letters, one to three bytes
    bad = text + b"x\xffy \xc3 \xe4\xb8 \xf0\x9f\x98z \xed\xa0\x80 \xc0\xaf \xef\xbf\xbd\xff\xfe ok\n"
    _check_against_file_routes(bad, 4, ("english", "numbers", "\ufffd"), ("\n", "."), tmp_path, "fffd")
    # sentences of one token: <S> w </S> has no 4-gram, so level 4 is empty; two-token sentences besides: level 5 of order 5 is
    for tag, t, order in (("single", b"alpha\nbeta\n\nalpha\nGamma.\n", 4), ("pairs", b"alpha beta\nbeta\nalpha beta\n", 6)):
        built = _check_against_file_routes(t, order, ALPHA_WIDE, ("\n",), tmp_path, tag)
        c, v, total = built["count"].level(order - 1)
        assert len(c) == 0 and len(v) == 0 and total == 0
        assert len(built["count"].level(2)[1]) > 0
    # no token at all, and no byte at all
    for tag, t in (("notoken", b"!!! ??? \n\n ;; \xff \n"), ("empty", b"")):
        built = _check_against_file_routes(t, 3, ("english",), ("\n",), tmp_path, tag)
        for m in built.values():
            assert len(m) == 0 and m.order == 3
            for c, v, total in _levels(m):
                assert len(c) == 0 and len(v) == 0 and total == 0


def test_multibyte_sequences_at_slice_boundaries(tmp_path):
    """whole, truncated and invalid sequences of 2, 3 and 4 bytes on every offset of a 16-byte boundary: the text is shifted
    byte by byte through sixteen alignments, and a second text puts a truncated sequence at offsets 0..3 behind a boundary"""
    alpha = ("english", "russian", "numbers", "世界é")
    core = ("Привет мир 世界 Ünï é\n" * 3).encode() + b"a\xd0 b\xe4\xb8 c\xf0\x9f\x98 d\xf0\x9f e\xe4\n" + "😀世😀д😀\n".encode() + \
        b"\x80\x80\x80\x80 f\xbf\xbf g\xe4\xb8\xe4\xb8\x96 \xd0\xd0\xbf\n" + ("дом " * 9).encode() + b"\xd0"
    for shift in range(16):
        _check_against_file_routes(b"x" * shift + b" " + core, 3, alpha, ("\n",), tmp_path, "shift%d" % shift)
    buf = b""
    for trunc in (b"\xd0", b"\xe4\xb8", b"\xf0\x9f\x98", b"\xf0\x9f"):
        for off in range(4):                                       # the sequence starts `off` bytes behind a 16-byte boundary
            buf += b"w" + b" " * ((off - len(buf) - 1) % 16 + 16)
            assert len(buf) % 16 == off
            buf += trunc + b"q "
    _check_against_file_routes(buf + b"\n", 3, alpha, ("\n",), tmp_path, "trunc")


def test_hash_collisions_are_told_apart_by_the_bytes(tmp_path):
    from suggest_amd import _lib
    from suggest_amd.spell import LanguageModel
    text = _messy_text()
    full = LanguageModel.from_corpus(text, 4, "<S>", "</S>", ALPHA_WIDE, SEPS_WIDE, id_order="count")
    full_lines = LanguageModel.from_corpus(text, 4, "<S>", "</S>", ALPHA_WIDE, SEPS_WIDE, id_order="lines")
    assert len(full) > 2                                           # 15 words: with 1 hash bit at least 13 of them meet a word of their hash
    L = _lib.lib()
    for bits in (4, 1):
        try:
            _lib.check(L.sg_debug_lm_build_hash_bits(bits))
            few = LanguageModel.from_corpus(text, 4, "<S>", "</S>", ALPHA_WIDE, SEPS_WIDE, id_order="count")
            few_lines = LanguageModel.from_corpus(text, 4, "<S>", "</S>", ALPHA_WIDE, SEPS_WIDE, id_order="lines")
        finally:
            _lib.check(L.sg_debug_lm_build_hash_bits(0))
        _assert_same(few, full, "%d hash bits, count" % bits)
        _assert_same(few_lines, full_lines, "%d hash bits, lines" % bits)
    prod = tmp_path / "prod"
    prod.mkdir()
    LanguageModel.build_files(text, str(prod), 4, "<S>", "</S>", ALPHA_WIDE, SEPS_WIDE)
    _assert_same(few, oracle.OracleLM(str(prod), 4, "<S>", "</S>", ALPHA_WIDE, id_order="count"), "1 hash bit, file route")
    assert L.sg_debug_lm_build_hash_bits(65) == -1


def _zipf_corpus(n_tokens, n_vocab, seed):
    """-> (text bytes, lines): Zipf-distributed words, one in twelve non-ASCII, some upper-cased in the text, sentences of 1..30 words"""
    rng = np.random.RandomState(seed)
    words = set()
    while len(words) < n_vocab:
        ln = rng.randint(2, 11, size=n_vocab)
        ch = rng.randint(0, 26, size=(n_vocab, 10))
        for i in range(n_vocab):
            w = "".join(chr(97 + int(c)) for c in ch[i, :ln[i]])
            if i % 12 == 0:
                w = w[:1] + "éжüя"[i // 12 % 4] + w[1:]
            words.add(w)
            if len(words) == n_vocab:
                break
    words = sorted(words)
    rng.shuffle(words)
    p = 1.0 / np.arange(1, n_vocab + 1) ** 1.05
    cdf = np.cumsum(p); cdf /= cdf[-1]
    draws = np.searchsorted(cdf, rng.random_sample(n_tokens))
    style = rng.randint(0, 20, size=n_tokens)                      # 0: UPPER, 1: Capitalised, else as it is
    lines, at = [], 0
    while at < n_tokens:
        n = int(rng.randint(1, 31))
        toks = []
        for j in range(at, min(at + n, n_tokens)):
            w = words[int(draws[j])]
            toks.append(w.upper() if style[j] == 0 else w.capitalize() if style[j] == 1 else w)
        lines.append(" ".join(toks))
        at += n
    return ("\n".join(lines) + "\n").encode(), lines


SIZE_ALPHA = ("english", "russian", "numbers", "éü")


def test_one_million_tokens(tmp_path):
    """1 000 000 tokens, a vocabulary of 50 000, order 3: multi-pass sorts, hot-word atomics (<S>, </S> and the first ranks of the
    Zipf law) and many workgroups per stage.  The oracle's build and load of this corpus take about ten seconds."""
    from suggest_amd.spell import LanguageModel
    text, _ = _zipf_corpus(1_000_000, 50_000, 5)
    ora = tmp_path / "ora"
    ora.mkdir()
    oracle.lm_build_files(text, str(ora), 3, "<S>", "</S>", SIZE_ALPHA, ("\n",))
    want = oracle.OracleLM(str(ora), 3, "<S>", "</S>", SIZE_ALPHA, id_order="count")
    dev = LanguageModel.from_corpus(text, 3, "<S>", "</S>", SIZE_ALPHA, ("\n",), id_order="count")
    assert len(dev) > 40_000
    _assert_same(dev, want, "1M tokens")


def test_spellchecker_and_scores_end_to_end(tmp_path):
    from suggest_amd.spell import LanguageModel, SpellChecker
    text, lines = _zipf_corpus(150_000, 8_000, 9)
    prod = tmp_path / "prod"
    prod.mkdir()
    LanguageModel.build_files(text, str(prod), 3, "<S>", "</S>", SIZE_ALPHA, ("\n",))
    a = LanguageModel.from_corpus(text, 3, "<S>", "</S>", SIZE_ALPHA, ("\n",), id_order="count")
    b = LanguageModel(str(prod), 3, "<S>", "</S>", SIZE_ALPHA, id_order="count")
    sa, sb = SpellChecker(a), SpellChecker(b)
    rng = np.random.RandomState(4)
    queries = []
    while len(queries) < 3000:                                     # two context words + a prefix (2 of 3) or a typo (1 of 3)
        ws = lines[int(rng.randint(0, len(lines)))].lower().split(" ")
        if len(ws) < 3:
            continue
        p = int(rng.randint(2, len(ws)))
        w = ws[p]
        if len(queries) % 3 == 2 and len(w) > 3:
            j = int(rng.randint(1, len(w)))
            w = w[:j] + chr(97 + int(rng.randint(0, 26))) + w[j + 1:]
        else:
            w = w[:max(2, (len(w) * 2 + 2) // 3)]
        queries.append(ws[p - 2] + " " + ws[p - 1] + " " + w)
    for k, sim in ((5, 0.5), (2, 0.3)):
        ia, ca = sa.predict_batch(queries, k, sim)
        ib, cb = sb.predict_batch(queries, k, sim)
        assert np.array_equal(ca, cb), (k, sim)
        assert np.array_equal(ia, ib), (k, sim)
        assert int((ca > 0).sum()) > len(queries) // 2
    some = lines[:400] + ["Unknownword zzzz " + lines[7], "", "  "]
    (s1, w1, u1), (s2, w2, u2) = a.score_text_batch(some), b.score_text_batch(some)
    assert np.array_equal(w1, w2) and np.array_equal(u1, u2)
    assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64))
    assert int(w1.sum()) > 400 and int(u1.sum()) >= 2


def test_save_after_build(tmp_path):
    from suggest_amd.spell import LanguageModel
    dev = LanguageModel.from_corpus(_messy_text(), 4, "<S>", "</S>", ALPHA_WIDE, SEPS_WIDE, id_order="count")
    lm_path, cdb_path = str(tmp_path / "built.lm"), str(tmp_path / "built.cdb")
    dev.save(lm_path, cdb_path)
    _assert_same(LanguageModel(binary=lm_path, dictionary=cdb_path, alphabet=ALPHA_WIDE), dev, "saved and reloaded")


def test_argument_errors():
    from suggest_amd import _lib
    L = _lib.lib()
    text = b"i am sam\n"
    alpha = (C.c_char_p * 1)(b"english")
    seps = (C.c_char_p * 1)(b"\n")
    buf = C.create_string_buffer(text, len(text))
    sentinel = 0x5A5A5A5A

    def call(length=len(text), order=3, start=b"<S>", end=b"</S>", alphabet=alpha):
        h = C.c_void_p(sentinel)
        rc = L.sg_lm_build_device(C.addressof(buf), length, order, start, end, alphabet, 1, seps, 1, 1, 0, C.byref(h))
        assert h.value == sentinel                                  # *out is left alone
        return rc, L.sg_last_error().decode()

    for kwargs, code, word in ((dict(order=0), -1, "nGramOrder"), (dict(order=9), -1, "nGramOrder"), (dict(start=b""), -1, "empty"),
                               (dict(end=b""), -1, "empty"), (dict(start=b"< S>"), -1, "space, tab or newline"),
                               (dict(end=b"a\tb"), -1, "space, tab or newline"), (dict(start=b"a\n"), -1, "space, tab or newline"),
                               (dict(length=(1 << 30) + 1), -2, "1 GiB")):
        assert L.sg_lm_load_google(b"/no/such/directory", 3, b"<S>", b"</S>", alpha, 1, C.byref(C.c_void_p())) == -1   # (another message in between)
        assert "1-gm" in L.sg_last_error().decode()
        rc, msg = call(**kwargs)
        assert rc == code and word in msg, (kwargs, rc, msg)
    rc, msg = call(alphabet=(C.c_char_p * 1)(b"ab c"))
    assert rc == -2 and "U+0020" in msg
