"""The three language-model paths on the device at every order the C ABI takes (1 .. 8) and with long contexts: Predict
(spell_tokenize_kernel -> spell_next_kernel -> the two searches -> spell_merge_kernel) against the oracle's Predict, sentence
scoring (lm_score.inc) against the host's one-sentence scorer, the corpus builder (lm_build.inc) against both file routes.
The host references are themselves held to the oracle by test_lm_orders_cpu.py.  Predict rows and builder arrays are compared
exactly; scores with test_gpu_lm_score._assert_close (1e-12 relative: device log() and glibc log() are not known to agree to the
bit), infinities and the exact zero equal.  Every `assert` on the inputs alone (how many queries of a kind the batch holds, that
the oracle's rows depend on a long context) keeps a test from going vacuous and is checked before the device is asked."""
import itertools

import numpy as np
import pytest

import oracle
from test_gpu_lm_build import ALPHA_WIDE, _check_against_file_routes
from test_gpu_lm_score import UNK, _assert_close, _host_ids, _score_ids, _tok_check
from test_lm_orders_cpu import ORPHAN_GRAMS, corpus_text, make_vocab, orphan_sentences, write_orphan_model, zipf_corpus
from test_spell import SPELL_INDEX, _assert_same_predictions

pytestmark = pytest.mark.gpu

ORDERS = (1, 2, 3, 4, 5, 6, 7, 8)
LM_ERROR = 0xFFFFFFFC               # SG_COUNT_LM_ERROR
BLOCK, STAGE_BYTES = 256, 12288     # spell_tokenize_kernel: queries of a block; query bytes a block stages in LDS (SG_STOK_BYTES)
ALPHA = ("english", "numbers")
# sixty short words in families that differ in a letter or two: a prefix has several completions, a typo has neighbours
VOCAB = make_vocab(["ba", "ca", "ma", "ta", "sa", "lo", "mi", "re", "do", "fu"], ["n", "t", "nd", "rk", "ller", "tion"])


@pytest.fixture(scope="module")
def corpus():
    return zipf_corpus(VOCAB, 400, 16, seed=31, families=150)


def _models(directory, text, order, alpha, index_alpha=None):
    """-> (LanguageModel, SpellChecker, OracleLM, OracleIndex) of the product's count files of `text`"""
    from suggest_amd import IndexDescription, LanguageModel, SpellChecker
    LanguageModel.build_files(text, directory, order, "<S>", "</S>", alpha, ("\n",))
    lm = LanguageModel(directory, order, alphabet=alpha)
    ora_lm = oracle.OracleLM(directory, order, alphabet=alpha)
    desc = dict(SPELL_INDEX, alphabet=index_alpha) if index_alpha else SPELL_INDEX
    sc = SpellChecker(lm, description=IndexDescription(name="words", **desc))
    return lm, sc, ora_lm, oracle.OracleIndex(ora_lm.words(), **desc)


def _assert_entry_points_agree(sc, qb, qo, k, sim):
    """the rows of predict_batch_device (queries and rows in HBM) equal those of the host-buffer entry point -> the counts"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(qo) - 1
    h_ids, h_cnt = sc.predict_batch(blob=qb, offs=qo, top_k=k, similarity=sim)
    d_q = torch.from_numpy(qb).to(dev); d_o = torch.from_numpy(qo.view(np.int64)).to(dev)
    d_ids = torch.full((n, k + 1), 7, dtype=torch.int32, device=dev); d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    sc.predict_batch_device(d_q.data_ptr(), d_o.data_ptr(), n, int(qo[-1]), k, sim, d_ids.data_ptr(), d_cnt.data_ptr(),
                            stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32), h_cnt)
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), h_ids)
    return h_cnt


def _mangle(word, kind, rnd):
    if kind == 0:
        return word[:int(rnd.randint(1, len(word)))]                   # a prefix
    if kind == 1 and len(word) > 2:
        p = int(rnd.randint(0, len(word)))
        return word[:p] + "x" + word[p + 1:]                            # a typo
    return word                                                         # whole


def _queries(sentences, n_queries, seed, unknown="zzunknown", max_window=15):
    """-> [(context words, last word)]: two in three are windows of corpus sentences with 0 .. max_window context words (seen contexts),
    one in three the tail of glued sentences with 9 .. 20 (partly unseen); one in six has an unknown word in the context, half
    of these among its last two words"""
    rnd = np.random.RandomState(seed)
    by_len = {n: [s for s in sentences if len(s) > n] for n in range(max_window + 1)}
    out = []
    for i in range(n_queries):
        if i % 3 < 2:
            n = int(rnd.randint(0, max_window + 1))
            s = by_len[n][int(rnd.randint(0, len(by_len[n])))]
            cut = int(rnd.randint(n, len(s)))                           # the last word's position
            ctx, word = list(s[cut - n:cut]), s[cut]
        else:
            n = int(rnd.randint(9, 21))
            s = []
            while len(s) < n + 1:
                s = s + sentences[int(rnd.randint(0, len(sentences)))]
            cut = int(rnd.randint(n, len(s)))
            ctx, word = list(s[cut - n:cut]), s[cut]
        if i % 6 == 1 and ctx:
            at = len(ctx) - 1 - int(rnd.randint(0, min(2, len(ctx)))) if i % 12 == 1 else int(rnd.randint(0, len(ctx)))
            ctx[at] = unknown
        out.append((ctx, _mangle(word, int(rnd.randint(0, 3)), rnd)))
    return out


def _text(q, i):
    t = " ".join(q[0] + [q[1]])
    return (t.upper() if i % 5 == 0 else t).encode()


def _arrange(queries):
    """-> the queries' indices in an order in which spell_tokenize_kernel takes both of its branches: the 256 heaviest queries fill the second
    block, and the batch starts with a query of odd length"""
    order = sorted(range(len(queries)), key=lambda i: -len(_text(queries[i], i)))
    heavy, light = order[:BLOCK], sorted(order[BLOCK:])
    odd = next(i for i in light if len(_text(queries[i], i)) % 2 == 1)
    light.remove(odd)
    light = [odd] + light
    return light[:BLOCK] + heavy + light[BLOCK:]


def _block_bytes(offs):
    starts = np.arange(0, len(offs) - 1, BLOCK)
    ends = np.minimum(starts + BLOCK, len(offs) - 1)
    return offs[starts].astype(np.int64), (offs[ends] - offs[starts]).astype(np.int64)


def _reaches_next(n, order):
    """the context positions LanguageModel.Next hands to NGramModel.Next (language_model.go:100-112), of n context words"""
    if n + 1 < order or n < order:
        return range(n)
    if n == order:
        return range(order - 1)                                         # (sic) the first order - 1 words
    return range(n - (order - 1), n)


@pytest.fixture(scope="module")
def batch(corpus):
    queries = _queries(corpus, 2048, seed=41)
    origin = _arrange(queries)
    return [queries[i] for i in origin], [_text(queries[i], i) for i in origin]


@pytest.mark.parametrize("order", ORDERS)
def test_predict_at_every_order_with_long_contexts(order, corpus, batch, tmp_path):
    queries, texts = batch
    lm, sc, ora_lm, ora_ix = _models(str(tmp_path), corpus_text(corpus), order, ALPHA)
    assert len(lm.level(order - 1)[1]) > 0
    N = order
    n_ctx = np.array([len(c) for c, _ in queries])
    # ---- conditions on the inputs, from the oracle alone ----
    if N >= 4:
        assert ((n_ctx + 1 < N) & (n_ctx >= 2)).sum() >= 20              # the start symbol in front of more than one context word
    assert (n_ctx == N).sum() >= 20                                      # (sic) the first N - 1 words
    if N <= 7:
        assert ((n_ctx > N) & (n_ctx <= 8)).sum() >= 20                  # trimmed, ids from the first eight tokens
    assert (n_ctx > 8).sum() >= 20                                       # trimmed, ids from the ring of the latest eight
    if N >= 2:
        assert sum("zzunknown" in c[max(0, len(c) - (N - 1)):] for c, _ in queries) >= 20
        assert sum(any(c[j] == "zzunknown" for j in _reaches_next(len(c), N)) for c, _ in queries) >= 20   # ... and is handed to Next
    qb, qo = oracle.pack_strings(texts)
    starts, sizes = _block_bytes(qo)
    assert (sizes > STAGE_BYTES).any() and (sizes <= STAGE_BYTES).any()  # a block that is staged in LDS and one that is not
    assert ((sizes <= STAGE_BYTES) & (starts % 4 != 0)).any()            # a staged block whose first byte is not dword-aligned
    assert len(texts[0]) % 2 == 1
    oi, oc = ora_lm.predict_batch(ora_ix, qb, qo, 5, 0.5)
    with_context = n_ctx > 0
    if N == 1:
        assert (oc[with_context] == LM_ERROR).all() and (oc[~with_context] != LM_ERROR).all()
    else:
        assert not (oc == LM_ERROR).any()
        bare = [t.split(b" ")[-1] for t in texts]                         # the last word alone: no context, no scorer
        bi, bc = ora_lm.predict_batch(ora_ix, *oracle.pack_strings(bare), 5, 0.5)
        reranked = (oc != bc) | (oi != bi).any(axis=1)
        assert (reranked & (n_ctx > 8)).sum() >= 10                       # a wrong id out of the ring would show in the rows
    # ---- the device ----
    for top_k, sim in ((5, 0.5), (2, 0.3)):
        _assert_same_predictions(sc, ora_lm, ora_ix, texts, top_k, sim)
    if N == 1:
        assert (sc.predict_batch(blob=qb, offs=qo, top_k=5, similarity=0.5)[1][with_context] == LM_ERROR).all()
    if N in (1, 5, 8):                                                   # the device-resident entry point gives the same rows
        _assert_entry_points_agree(sc, qb, qo, 5, 0.5)


RU_VOCAB = make_vocab(["ко", "до", "ма", "сте", "пе", "зи"], ["т", "м", "н", "рка", "лка"]) + \
    ["webсайт", "webсад", "eмail", "ёжик", "ёлка", "ежик", "дом2", "domик", "кот", "код"]


@pytest.mark.parametrize("order", (2, 5))
def test_predict_over_a_non_ascii_vocabulary(order, tmp_path):
    """Cyrillic and mixed words, queries in upper and mixed case: d_lm_lower on letters, the multi-byte re-encoding into the
    slot, d_word_id on multi-byte words, a non-ASCII last word into the two searches"""
    alpha = ("english", "russian", "numbers")
    sentences = zipf_corpus(RU_VOCAB, 300, 12, seed=51, families=80)
    lm, sc, ora_lm, ora_ix = _models(str(tmp_path), corpus_text(sentences), order, alpha)
    assert sorted(w.decode() for w in lm.words() if not w.startswith(b"<")) == sorted(set(RU_VOCAB))
    queries = _queries(sentences, 768, seed=52, unknown="неттакого", max_window=11)
    texts = []
    for i, (ctx, word) in enumerate(queries):
        t = " ".join(ctx + [word])
        t = t.upper() if i % 3 == 0 else "".join(c.upper() if (i + j) % 2 else c for j, c in enumerate(t)) if i % 3 == 1 else t
        texts.append(t.encode())
    assert sum(t != t.lower() for t in (x.decode() for x in texts)) > 400
    qb, qo = oracle.pack_strings(texts)
    oi, oc = ora_lm.predict_batch(ora_ix, qb, qo, 5, 0.5)
    assert ((oc > 0) & (oc < LM_ERROR)).sum() > len(texts) // 2          # most queries have predictions
    bi, bc = ora_lm.predict_batch(ora_ix, *oracle.pack_strings([t.split(b" ")[-1] for t in texts]), 5, 0.5)
    assert ((oc != bc) | (oi != bi).any(axis=1)).sum() >= 10             # the Cyrillic context words are found: rows depend on them
    for top_k, sim in ((5, 0.5), (2, 0.3)):
        _assert_same_predictions(sc, ora_lm, ora_ix, texts, top_k, sim)


FFFD_ALPHA = ("english", "numbers", "\ufffd")
# (every invalid byte is one U+FFFD: words of one to four replacement runes, two of them with letters — six different words)
FFFD_WORDS = [b"\xff", b"\xff\xfe", b"\xc3", b"\xe4\xb8", b"\xf0\x9f\x98", b"a\xff", b"\xffb\xfe", b"\xff\xff\xff\xff", b"\xed\xa0\x80", b"\xc0\xaf"]


def _fffd_corpus():
    rnd = np.random.RandomState(61)
    vocab = [w.encode() for w in VOCAB[:20]] + FFFD_WORDS
    return [b" ".join(vocab[int(i)] for i in rnd.randint(0, len(vocab), size=int(rnd.randint(1, 9)))) for _ in range(300)]


def test_predict_with_the_replacement_rune_as_a_letter(tmp_path):
    """U+FFFD in the model's alphabet: an invalid byte of a query becomes a letter of three bytes, so a query's slot holds three
    bytes per query byte (slot_mul).  Queries of invalid bytes sit between ordinary ones, whose rows are compared as well: with
    a slot of two bytes per byte such a query wrote over its neighbour's tokens."""
    lines = _fffd_corpus()
    lm, sc, ora_lm, ora_ix = _models(str(tmp_path), b"\n".join(lines) + b"\n", 3, FFFD_ALPHA, index_alpha=("english", "numbers", "$^'\ufffd"))
    assert sum(b"\xef\xbf\xbd" in w for w in lm.words()) >= 6
    rnd = np.random.RandomState(62)
    bad, plain = [], []
    for i in range(301):                                                 # context words and last words of invalid bytes only
        ws = [FFFD_WORDS[int(j)] for j in rnd.randint(0, len(FFFD_WORDS), size=int(rnd.randint(1, 5)))]
        if i % 4 == 0:
            ws[-1] = ws[-1] + b"\xfe\xfd"[:int(rnd.randint(0, 3))]       # not quite a word of the model: the fuzzy search
        bad.append(b" ".join(ws))
    for i in range(300):
        line = [w for w in lines[int(rnd.randint(0, len(lines)))].split(b" ") if w.isalpha()] or [VOCAB[i % 20].encode()]
        if 128 <= i < 256:                                               # long ordinary queries: the second block is not staged
            line = line[:-1] + lines[int(rnd.randint(0, len(lines)))].split(b" ") + [w.encode() for w in VOCAB[20:36]] + line[-1:]
        plain.append(b" ".join(line[:-1] + [line[-1][:max(2, len(line[-1]) - 1)]]))
    texts = [bad[i // 2] if i % 2 == 0 else plain[i // 2] for i in range(601)]   # bad first in the blocks 0, 1 and 2, and last in the batch
    grown = np.array([sum(len(x) for x in lm.Tokenize(t)) / len(t) for t in texts[0::2]])
    assert (grown > 2.0).sum() > 200 and grown.max() <= 3.0              # tokens that do not fit two bytes per query byte; three hold all
    qb, qo = oracle.pack_strings(texts)
    starts, sizes = _block_bytes(qo)
    assert (3 * sizes <= 2 * STAGE_BYTES).any() and (3 * sizes > 2 * STAGE_BYTES).any()   # staged at three bytes of slot per byte, and not
    oi, oc = ora_lm.predict_batch(ora_ix, qb, qo, 5, 0.5)
    assert (oc[0::2] > 0).sum() > 200 and (oc[1::2] > 0).sum() > 200
    for top_k, sim in ((5, 0.5), (2, 0.3)):
        _assert_same_predictions(sc, ora_lm, ora_ix, texts, top_k, sim)
    assert np.array_equal(_assert_entry_points_agree(sc, qb, qo, 5, 0.5), oc)


# ---- sentence scoring at orders 4 .. 8 ----
def _score_both_paths(lm, lists, order, what):
    """the ids path and the text path of `lists` against the host's scorer -> (device scores of the ids path, the host's)"""
    dev = _score_ids(lm, lists)
    host = np.array([_host_ids(lm, s) for s in lists])
    _assert_close(dev, host, what)
    empty = np.array([len(s) + 2 < order for s in lists])
    assert empty.any() and (dev[empty] == 0.0).all() and not np.signbit(dev[empty]).any()   # no window: exactly +0.0
    V = len(lm)
    name = lambda w: lm.word(w) if w < V else b"qqunknown"
    lines = [b" ".join(name(w) for w in s) for s in lists if all(w < V or w == UNK for w in s)]
    assert len(lines) > len(lists) // 2
    _tok_check(lm, lines)
    return dev, host


@pytest.mark.parametrize("order", (4, 5, 6, 7, 8))
def test_scores_on_the_corpus_model(order, corpus, tmp_path):
    lm = _models(str(tmp_path), corpus_text(corpus), order, ALPHA)[0]
    assert len(lm.level(order - 1)[1]) > 0
    V = len(lm)
    rnd = np.random.RandomState(70 + order)
    vocab = [lm.GetWordID(w) for w in VOCAB[:5]] + [UNK, V + 2]          # a slice of the vocabulary, an unknown id, one past the words
    lists = [list(c) for n in range(5) for c in itertools.product(vocab, repeat=n)]
    lists += [[lm.GetWordID(w) for w in s] for s in corpus[:200]]        # seen: hits on every level
    for s in corpus[200:400]:                                            # a miss somewhere: back-off from deep prefixes
        ids = [lm.GetWordID(w) for w in s]
        ids[int(rnd.randint(0, len(ids)))] = [UNK, V, int(rnd.randint(0, V))][int(rnd.randint(0, 3))]
        lists.append(ids)
    lists += [[UNK if w == V else int(w) for w in rnd.randint(0, V + 1, size=int(rnd.randint(0, 21)))] for _ in range(200)]
    _score_both_paths(lm, lists, order, "corpus model, order %d" % order)


@pytest.mark.parametrize("order", (4, 5, 6, 7, 8))
def test_scores_on_the_orphan_model(order, tmp_path):
    from suggest_amd import LanguageModel
    write_orphan_model(str(tmp_path))
    lm = LanguageModel(str(tmp_path), order)
    assert [len(lm.level(k)[1]) for k in range(1, order)] == [len(ORPHAN_GRAMS[k + 1]) for k in range(1, order)]
    V = len(lm)
    vocab = list(range(V)) + [UNK, V + 3]
    lists = [list(c) for n in range(5) for c in itertools.product(vocab, repeat=n)] + orphan_sentences(lm, order, 600)
    dev, host = _score_both_paths(lm, lists, order, "orphan model, order %d" % order)
    assert np.isinf(host).any() and np.array_equal(np.isinf(dev), np.isinf(host))


def test_scores_of_a_long_sentence_among_short_ones_at_order_eight(corpus, tmp_path):
    """a sentence of 700 words between short ones in one workgroup: its windows cross the rounds of 256 windows, and the short
    sentences' windows share those rounds with its first and last ones"""
    lm = _models(str(tmp_path), corpus_text(corpus), 8, ALPHA)[0]
    rnd = np.random.RandomState(81)
    ids = [[lm.GetWordID(w) for w in s] for s in corpus]
    long_one = [w for s in ids[:80] for w in s][:700]
    assert len(long_one) == 700
    shorts = [ids[int(i)][:int(rnd.randint(0, 17))] for i in rnd.randint(0, len(ids), size=40)]
    for lists in (shorts[:20] + [long_one] + shorts[20:], [long_one] + shorts, shorts + [long_one], [long_one, long_one[::-1], long_one[3:]]):
        dev = _score_ids(lm, lists)
        _assert_close(dev, np.array([_host_ids(lm, s) for s in lists]), "long sentence")
        _tok_check(lm, [b" ".join(lm.word(w) for w in s) for s in lists])


def test_scores_with_the_replacement_rune_as_a_letter(tmp_path):
    """the text path on a model whose alphabet holds U+FFFD (lm_upload: three bytes of slot per byte of a line): lines of invalid
    bytes next to ordinary lines"""
    lines = _fffd_corpus()
    lm = _models(str(tmp_path), b"\n".join(lines) + b"\n", 4, FFFD_ALPHA)[0]
    rnd = np.random.RandomState(91)
    batch_lines = []
    for i in range(600):
        if i % 2 == 0:
            n = int(rnd.randint(1, 12))
            batch_lines.append(b" ".join(FFFD_WORDS[int(j)] for j in rnd.randint(0, len(FFFD_WORDS), size=n)) + b"\xff" * int(rnd.randint(0, 3)))
        else:
            batch_lines.append(lines[int(rnd.randint(0, len(lines)))].upper())
    batch_lines += [b"\xff" * 200, b"", b"\xfe", lines[0]]
    s, w, u = _tok_check(lm, batch_lines)
    assert w[600] == 1 and u[600] == 1 and (u[:600:2] < w[:600:2]).sum() > 250   # words of U+FFFD are found in the vocabulary


# ---- the builder with entries on the levels 5 .. 8 ----
@pytest.mark.parametrize("order", (5, 7, 8))
def test_builder_with_full_upper_levels(order, corpus, tmp_path):
    """the keys ctx[k-1][p] << 32 | word and the radix sort's bits in use are widest on the top levels"""
    built = _check_against_file_routes(corpus_text(corpus), order, ALPHA_WIDE, ("\n",), tmp_path, "o%d" % order)
    for m in built.values():
        assert len(m.level(order - 1)[1]) > 100
