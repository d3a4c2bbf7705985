"""The descriptions, texts and dictionary of tests/tokenizer_shapes.py against the CPU oracle alone (no GPU): the host
tokeniser and CSR builder agree with the oracle on every one of them, the texts reach the edges the device tests are about —
otherwise a device test could pass without ever meeting a short gram, a trimmed text or a 128-gram query — and the oracle's own
rows are worth comparing (none flagged, nine in ten hold a result).  Conditions on the inputs, not measurements of the product."""
import pytest

import oracle
import tokenizer_shapes as ts

AT_LEAST = 3
CAN, CANNOT = "can", "cannot"

# What a description cannot produce from these texts, and why; every class not named is one it can (AT_LEAST texts).
#   no_0:    the lower-cased, trimmed wrap alone has q bytes or more: the n-gram tokeniser's last append always yields a gram
#   no_1:    ... and q + 1 runes or more, whose first two grams differ: two tokens at least
#   no_short: a short gram needs bytes >= q > runes; the wrap alone has q - 1 runes or more (or q = 1: runes >= bytes >= 1)
#   no_trim: neither end of the wrap is a space, so strings.Trim finds nothing
#   q1_tokens: q = 1: a token per distinct rune; no pool has more than 17, a spliced sequence adds 4 at most
#   wrap8: text of L runes -> L + 14 grams; 63-65 and 127-129 need L = 49-51 and 113-115, lengths the lists do not hold (an
#          ill-formed splice adds at most 4 runes to 40 or 70; the dedup-edge walks have 128)
_NO_TRIM = ("trimmed",)
CANNOT_TABLE = {
    "q1-nowrap": ("tokens_127_129", "short_gram"),                                   # q1_tokens, no_short (q = 1)
    "q2-dollar": ("tokens_0", "short_gram") + _NO_TRIM,                              # no_0 ("$$"), no_short
    "q3-wrap8": ("tokens_0", "tokens_1", "grams_63_65", "grams_127_129", "short_gram") + _NO_TRIM,   # no_0, no_1, wrap8
    "q3-upper-wrap-pad-e": ("tokens_0", "tokens_1", "short_gram") + _NO_TRIM,        # "ab z": "ab ", "b z"
    "q2-space-wrap": (),                                                             # the wrap is trimmed away: everything is open
    "q3-wrap-widths": ("tokens_0", "tokens_1", "short_gram") + _NO_TRIM,             # "ikⱥ$": "ikⱥ", "kⱥ$"
    "q4-guillemets": ("tokens_0",) + _NO_TRIM,                                       # "«»" is four bytes, two runes
    "q2-pad4": ("tokens_0", "short_gram") + _NO_TRIM,
    "q4-pad2": _NO_TRIM,                                                             # "$$": two bytes, so tokens_0 and short grams exist
    "q8-cyrillic-wrap": _NO_TRIM,
    "q5-space-wrap-nopad": (),
    "q1-pad-e": ("tokens_127_129", "short_gram"),
    "q3-fffd": ("tokens_0",) + _NO_TRIM,                                             # the wrap alone: six bytes, two runes (a short gram)
    "q3-unreachable-alphabet": ("short_gram",) + _NO_TRIM,                           # "$$" + one rune = q runes: never fewer with q bytes
    "synth": ("short_gram",) + _NO_TRIM,
}


def expectation(name, cls):
    return CANNOT if cls in CANNOT_TABLE[name] else CAN


@pytest.fixture(scope="module", params=ts.NAMES)
def described(request):
    d = ts.description(request.param)
    return request.param, d, oracle.OracleIndex(ts.dictionary(d), **d)


def test_the_inputs_are_what_the_issue_describes():
    assert len(ts.DESCRIPTIONS) == 15 and len(set(ts.NAMES)) == 15
    assert sum(u for _, _, u in ts.DESCRIPTIONS) == 6                   # five plan2-usable ones and the control
    a, u = ts.ascii_texts(1), ts.unicode_texts(2)
    assert len(a) == 6 + 3 * len(ts.ASCII_LENGTHS) == 255 and len(u) == 7 + 7 * ts.PER_POOL == 427
    assert [len(t) for t, _ in a[6:]] == [n for n in ts.ASCII_LENGTHS for _ in range(3)]
    assert all(set(t) <= set(p.encode()) for t, p in a[6:])
    assert sum(not ts._well_formed(t) for t, _ in u) == 7 * 18           # three strings in ten
    docs, qs = ts.dictionary(), ts.queries()
    t, e = ts.texts()
    assert len(docs) == ts.N_DOCS > 4 << 11 and docs[0] == ts.FIRST_DOC and docs[1:1 + len(qs)] == qs == t + e
    assert all(x != y for x, y in zip(t, e))
    w = ts.dedup_edge_texts(5)
    assert len(w) == ts.DEDUP_EDGE >= AT_LEAST and all(len(x) == 128 and x.strip(b" ") == x for x, _ in w)
    assert all(len({x.lower()[i:i + 2] for i in range(127)}) == 127 for x, _ in w)        # every bigram of a walk once
    assert ts.dictionary() is docs and ts.texts()[0] == [x for x, _ in a + u + w]      # seeded: the same on every call
    assert all(3 <= len(d.decode()) <= 20 for d in docs[1 + len(qs):])


def test_host_tokeniser_is_the_oracles(described):
    from suggest_amd import IndexDescription, NGramIndex
    name, d, ora = described
    host = NGramIndex([ts.FIRST_DOC], IndexDescription(**d), upload=False)
    for t in ts.queries(d) + ts.prefixes():
        for autocomplete in (False, True):
            assert host.tokenize(t, autocomplete) == ora.tokenize(t, autocomplete), (name, t, autocomplete)


def test_host_lists_are_the_oracles(described):
    from suggest_amd import IndexDescription, NGramIndex
    name, d, ora = described
    mine = NGramIndex(ts.dictionary(d), IndexDescription(**d), upload=False).lists()
    want = ora.lists()
    assert set(mine) == set(want)
    for key, (raw_len, post) in want.items():
        assert mine[key] == (raw_len, sorted(set(post))), (name, key)


def test_the_texts_reach_the_edges(described):
    name, d, ora = described
    c = ts.classes(ora, d, ts.queries(d))
    print(name, c)
    for cls in ts.CLASSES:
        if expectation(name, cls) == CAN:
            assert c[cls] >= AT_LEAST, (name, cls, c)
        else:
            assert c[cls] == 0, (name, cls, c)


def test_the_oracles_rows_are_worth_comparing(described):
    name, d, ora = described
    cnt = ora.suggest_batch(*oracle.pack_strings(ts.queries(d)), "jaccard", 0.3, 10)[2]
    flagged, share = ts.filled(cnt)
    print(name, len(cnt), flagged, share)
    assert flagged == 0 and share >= 0.9, (name, flagged, share)


def test_the_oracles_autocomplete_rows_are_worth_comparing(described):
    """six of the eleven prefix lengths drawn are nine runes or more, and half the texts are that long: such a prefix completes
    to its own text at least, under every description (q = 8 with its wrap needs seven runes) — a quarter of the rows at the least"""
    name, d, ora = described
    cnt = ora.autocomplete_batch(*oracle.pack_strings(ts.prefixes()), 80)[1]
    flagged, share = ts.filled(cnt)
    print(name, len(cnt), flagged, share)
    assert flagged == 0 and share >= 0.25, (name, flagged, share)


def test_the_interleaved_order_pairs_simple_with_other_queries():
    qs = ts.queries()
    for name, d, usable in ts.DESCRIPTIONS:
        order = ts.interleaved(d, qs)
        if not usable:
            continue

        def plan2_takes(t):          # plan2.inc: ASCII, at most 32 bytes and 48 runes with the wrap, nothing to trim, 2 .. 32 grams
            s = d["wrap"][0].encode() + t + d["wrap"][1].encode()
            g = len(s) - d["ngram_size"] + 1
            return all(b < 0x80 for b in s) and len(t) <= 32 and len(s) <= 48 and s.strip(b" ") == s and (len(s) < d["ngram_size"] or 2 <= g <= 32)

        pairs = [(plan2_takes(qs[order[i]]), plan2_takes(qs[order[i + 1]])) for i in range(0, len(order) - 1, 2)]
        if name == "q2-space-wrap":                                     # the wrap is a space: no query is simple
            assert not any(a or b for a, b in pairs)
            continue
        assert pairs.count((True, False)) >= 20 and pairs.count((False, True)) >= 20, (name, pairs.count((True, False)), pairs.count((False, True)))


def test_the_two_lower_case_tables_hold_the_same_pairs():
    """suggest_amd/csrc/unicode_lower.inc (from unicodedata) and oracle/unicode_lower.inc (from glibc's towlower) are generated
    independently; tests/test_gpu_case_table.py sends every pair of the first through d_lower against the second"""
    import os
    mine = ts.lower_pairs(os.path.join(oracle.ROOT, "suggest_amd", "csrc", "unicode_lower.inc"))
    theirs = ts.lower_pairs(os.path.join(oracle.ROOT, "oracle", "unicode_lower.inc"))
    assert len(mine) == 1364 and mine == theirs
    assert [a for a, _ in mine] == sorted({a for a, _ in mine}) and all(a >= 0x80 and a != b for a, b in mine)
    assert all(oracle.to_lower(chr(a).encode() + b"\xc2\xa0")[:-2] == chr(b).encode() for a, b in mine)


def test_the_chunks_cover_the_lower_case_table():
    import os
    pairs = ts.lower_pairs(os.path.join(oracle.ROOT, "suggest_amd", "csrc", "unicode_lower.inc"))
    chunks = ts.lower_chunks(pairs)
    assert [p for c in chunks for p in c] == pairs and all(0 < len(c) <= ts.LOWER_CHUNK for c in chunks)
    for c in chunks:
        docs, qs, near = ts.lower_chunk_strings(c, pairs)
        assert len(docs) == len(qs) == len(c) and len(near) > 0
        assert all(oracle.to_lower(q) == d for q, d in zip(qs, docs))
        assert oracle.to_lower(near) == near                  # what the table does not map stays as it is
