"""Shared by tests/test_tokenizer_shapes_cpu.py and tests/test_gpu_tokenizers.py: fifteen index descriptions (wraps of up to
eight runes, upper-case, spaced and non-ASCII wraps, pads of zero to four runes, q = 1 .. 8, alphabets beyond ASCII and beyond
the BMP), texts that put every device tokeniser on its edges (lengths around 32, 64 and 128 n-grams, heavy dedup, trimmed
ends, ill-formed UTF-8, runes whose lower case has another byte width), and a dictionary of the texts, their edited copies and
filler, large enough for the pipeline.  Everything is seeded; the yardstick is the CPU oracle (oracle/suggest_oracle.cpp), and
classes() says — from the oracle alone — how many texts of every kind a description's query list holds."""
import random

import numpy as np

import oracle
from suggest_amd import synth

SPECIAL = 0xFFFFFFF0                      # counts at and above flag a query the reference panics or dead-locks on
N_DOCS = 8400                             # the pipeline takes dictionaries above 4 << SG_LOG2_CNT = 8 192 documents
FIRST_DOC = b"abcabcab"                   # the reference panics if the first document has no tokens (indexer_writer.go:70)


def _d(q, wrap, pad, alphabet):
    return dict(ngram_size=q, wrap=wrap, pad=pad, alphabet=alphabet)


# (name, description, plan2-usable: ASCII wrap, one pad rune, q <= 3 — capi.inc, plan2_usable)
DESCRIPTIONS = (
    ("q1-nowrap", _d(1, ("", ""), "$", ("english", "numbers")), True),
    ("q2-dollar", _d(2, ("$", "$"), "$", ("english", "numbers", "$")), True),
    ("q3-wrap8", _d(3, ("^^^^^^^^", "$$$$$$$$"), "_", ("english", "_^$")), True),
    ("q3-upper-wrap-pad-e", _d(3, ("Ab", " z"), "é", ("english",)), True),
    ("q2-space-wrap", _d(2, (" ", " "), "_", ("english", "numbers", "_")), True),
    ("q3-wrap-widths", _d(3, ("İK", "Ⱥ$"), "$", ("english", "russian", "numbers", "$ⱥ")), False),
    ("q4-guillemets", _d(4, ("«", "»"), "·", ("english", "éèêàçœß", "«»·")), False),
    ("q2-pad4", _d(2, ("$", "$"), "$$$$", ("english", "$")), False),
    ("q4-pad2", _d(4, ("$", "$"), "é_", ("english", "$_é")), False),
    ("q8-cyrillic-wrap", _d(8, ("Ж", "ж"), "$", ("russian", "english", "$")), False),
    ("q5-space-wrap-nopad", _d(5, ("  ", " x "), "", ("english", "𝒳𝒴😀", "numbers")), False),
    ("q1-pad-e", _d(1, ("", ""), "é", ("ab",)), False),
    ("q3-fffd", _d(3, ("�", "�"), "�", ("english", "�")), False),
    ("q3-unreachable-alphabet", _d(3, ("$", "$"), "$", ("english", "KÅ", "$")), False),
    ("synth", dict(synth.DESCRIPTION), True),
)
NAMES = tuple(n for n, _, _ in DESCRIPTIONS)
# just over the 8-symbol term key (q x pad runes = 9 and 10): the host refuses them, on both build routes
OVER_THE_KEY = (_d(3, ("$", "$"), "$$$", ("english", "$")), _d(5, ("$", "$"), "é_", ("english", "$_é")))


def description(name):
    return next(d for n, d, _ in DESCRIPTIONS if n == name)


ASCII_LENGTHS = tuple(range(0, 41)) + tuple(range(60, 71)) + tuple(range(120, 151))
ASCII_POOLS = ("ab", "abcdeXYZ019 -.$^_")
UNICODE_FIXED = ("é", "éa", " é ", "😀", "İ", "Ⱥ", "K")
UNICODE_POOLS = ("abcXYZ -", "éÈœŒßẞ aB", "İıIiKkÅå", "ⱥȺȾⱦ ab", "жЖёЁ яab", "𝒳😀a b€", "ǅǄǆ Σσς")
UNICODE_COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 40, 63, 64, 65, 66, 70, 120, 127, 128, 129, 130, 135, 136, 137, 140, 143, 144, 145, 150, 200)
ILL_FORMED = (b"\xff", b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xed\xa0\x80", b"\xc0\xaf", b"\xf4\x90\x80\x80")
PER_POOL = 60


def _draw(rnd, pool, n):
    return "".join(rnd.choice(pool) for _ in range(n))


def ascii_texts(seed=1):
    """-> [(bytes, pool)]: the fixed strings, then three strings of every length of ASCII_LENGTHS"""
    rnd = random.Random(seed)
    out = [(t, ASCII_POOLS[1]) for t in (b"", b" ", b"  ", b" lead", b"trail ", b" both ")]
    for n in ASCII_LENGTHS:
        out.append((_draw(rnd, ASCII_POOLS[0], n).encode(), ASCII_POOLS[0]))
        out += [(_draw(rnd, ASCII_POOLS[1], n).encode(), ASCII_POOLS[1]) for _ in range(2)]
    return out


def unicode_texts(seed=2):
    """-> [(bytes, pool)]: the fixed strings, then PER_POOL strings of every pool; three in ten with an ill-formed sequence"""
    rnd = random.Random(seed)
    out = [(t.encode(), UNICODE_POOLS[1]) for t in UNICODE_FIXED]
    for pool in UNICODE_POOLS:
        for i in range(PER_POOL):
            t = _draw(rnd, pool, rnd.choice(UNICODE_COUNTS)).encode()
            if i % 10 < 3:
                at = rnd.randint(0, len(t))
                t = t[:at] + rnd.choice(ILL_FORMED) + t[at:]
            out.append((t, pool))
    return out


DEDUP_EDGE = 4                            # texts of dedup_edge_texts
DEDUP_EDGE_RUNES = 128


def dedup_edge_texts(seed=5):
    """-> [(bytes, pool)]: DEDUP_EDGE walks of 128 runes over the 17-symbol pool whose 127 bigrams are all distinct (no space at
    either end, so nothing is trimmed): under q = 2 the random texts stop near 118 distinct bigrams at 150 runes, and 127 - 129
    tokens after dedup — the wavefront kernel's last sizes — would go untried; a "$" wrap adds two bigrams at most"""
    rnd = random.Random(seed)
    pool = ASCII_POOLS[1]
    assert len(set(pool.lower())) == len(pool)
    out = []
    while len(out) < DEDUP_EDGE:
        t, seen = rnd.choice(pool.replace(" ", "")), set()
        while len(t) < DEDUP_EDGE_RUNES:
            fresh = [c for c in pool if (t[-1].lower(), c.lower()) not in seen and not (c == " " and len(t) == DEDUP_EDGE_RUNES - 1)]
            if not fresh:
                break                                         # (a dead end of the walk: start again)
            c = rnd.choice(fresh)
            seen.add((t[-1].lower(), c.lower()))
            t += c
        if len(t) == DEDUP_EDGE_RUNES:
            out.append((t.encode(), pool))
    return out


def _edit(rnd, text, pool):
    """a copy with one rune replaced by another of the pool (an ill-formed byte counts as a rune; an empty text gains one)"""
    runes = list(text.decode("utf-8", "surrogateescape"))
    if not runes:
        return rnd.choice(pool).encode()
    at = rnd.randrange(len(runes))
    runes[at] = rnd.choice([c for c in pool if c != runes[at]])
    return "".join(runes).encode("utf-8", "surrogateescape")


_CACHE = {}


def texts(seed=1):
    """-> (texts, edited copies), lists of bytes in step with one another: ascii_texts, unicode_texts, dedup_edge_texts"""
    if ("texts", seed) not in _CACHE:
        both = ascii_texts(seed) + unicode_texts(seed + 1) + dedup_edge_texts(seed + 4)
        rnd = random.Random(seed + 2)
        _CACHE["texts", seed] = ([t for t, _ in both], [_edit(rnd, t, p) for t, p in both])
    return _CACHE["texts", seed]


def queries(desc=None, seed=1):
    """every text, then every edited copy (the same list for every description)"""
    t, e = texts(seed)
    return t + e


def dictionary(desc=None, seed=1):
    """FIRST_DOC, the texts, their edited copies, then filler of 3 - 20 runes from the same pools: N_DOCS documents"""
    if ("dict", seed) not in _CACHE:
        t, e = texts(seed)
        docs = [FIRST_DOC] + t + e
        rnd = random.Random(seed + 3)
        pools = ASCII_POOLS + UNICODE_POOLS
        while len(docs) < N_DOCS:
            docs.append(_draw(rnd, rnd.choice(pools), rnd.randint(3, 20)).encode())
        _CACHE["dict", seed] = docs
    return _CACHE["dict", seed]


def prefixes(seed=1):
    """autocomplete queries: prefixes of the texts, cut at a rune boundary or (one in eight) inside a rune"""
    if ("prefixes", seed) not in _CACHE:
        rnd = random.Random(seed + 5)
        out = []
        for t in texts(seed)[0]:
            runes = list(t.decode("utf-8", "surrogateescape"))
            cut = "".join(runes[:rnd.choice((1, 2, 3, 4, 6, 9, 31, 64, 127, 129, 140))]).encode("utf-8", "surrogateescape")
            if rnd.randrange(8) == 0 and len(cut) > 1:
                cut = cut[:-1]
            out.append(cut)
        _CACHE["prefixes", seed] = out
    return _CACHE["prefixes", seed]


def interleaved(desc, qs):
    """the query list reordered so that simple ASCII queries (what sg_plan2_kernel's half-wavefront path takes: ASCII, at most 32
    bytes, nothing to trim) and the others alternate, the pairing shifted by one half-way through: with SG_ORDER=0 a wavefront
    of the plan2 launch then holds one of each, the simple one in its lower half in the first part and in its upper half in the second"""
    w0, w1 = desc["wrap"]

    def simple(t):
        s = w0.lower().encode() + t.lower() + w1.lower().encode()
        return len(t) <= 32 and all(b < 0x80 for b in t) and not (s[:1] == b" " or s[-1:] == b" ")

    a = [i for i, t in enumerate(qs) if simple(t)]
    b = [i for i, t in enumerate(qs) if not simple(t)]
    order = []
    n = min(len(a), len(b))
    for j in range(n):
        order += [a[j], b[j]] if j < n // 2 else [b[j], a[j]]
    order += a[n:] + b[n:]
    assert sorted(order) == list(range(len(qs)))
    return order


CLASSES = ("tokens_0", "tokens_1", "grams_31_33", "grams_63_65", "grams_127_129", "tokens_127_129", "dedup_dropped", "trimmed",
           "ill_formed", "width_changed", "short_gram")


def _well_formed(t):
    try:
        t.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def classes(ix, desc, qs):
    """-> {class: number of texts of qs in it}, counted with the oracle: `ix` an OracleIndex of `desc` (its tokenize), plus
    oracle.to_lower for what the n-gram tokeniser is handed (wrap, lower-case, trim: filter_tokenizer.go:20-27)"""
    q = desc["ngram_size"]
    c = dict.fromkeys(CLASSES, 0)
    for t in qs:
        wrapped = desc["wrap"][0].encode() + t + desc["wrap"][1].encode()
        low = oracle.to_lower(wrapped)
        s = low.strip(b" ")
        runes = len(s.decode("utf-8"))                       # (lower-casing a non-ASCII text re-encodes it: always well-formed; an ASCII one is)
        grams = 0 if len(s) < q else max(runes - q + 1, 1)   # ngram_tokenizer.go:18 and :41 (the last append happens whatever the length)
        tokens = len(ix.tokenize(t))
        assert tokens <= grams
        c["tokens_0"] += tokens == 0
        c["tokens_1"] += tokens == 1
        c["grams_31_33"] += 31 <= grams <= 33
        c["grams_63_65"] += 63 <= grams <= 65
        c["grams_127_129"] += 127 <= grams <= 129
        c["tokens_127_129"] += 127 <= tokens <= 129
        c["dedup_dropped"] += tokens < grams
        c["trimmed"] += len(s) != len(low)
        c["ill_formed"] += not _well_formed(t)
        c["width_changed"] += _well_formed(t) and any(len(oracle.to_lower(ch.encode() + b"\xc2\xa0")) - 2 != len(ch.encode()) for ch in set(t.decode()))
        c["short_gram"] += len(s) >= q > runes
    return c


def filled(counts):
    """(rows flagged, share of rows that hold a result)"""
    counts = np.asarray(counts)
    return int((counts >= SPECIAL).sum()), float(((counts > 0) & (counts < SPECIAL)).mean())


def lower_pairs(path):
    """the {from, to} pairs of a unicode_lower.inc (the device's table: suggest_amd/csrc; the oracle's: oracle/), in file order"""
    import re
    with open(path, encoding="utf-8") as f:
        text = f.read()
    pairs = [(int(a, 16), int(b, 16)) for a, b in re.findall(r"\{0x([0-9A-Fa-f]+),\s*0x([0-9A-Fa-f]+)\}", text)]
    assert len(pairs) == int(re.search(r"#define SG_UNICODE_LOWER_COUNT (\d+)", text).group(1))
    return pairs


LOWER_CHUNK = 240                         # alphabet + pad stay under the 255 distinct runes of the symbol table


def lower_chunks(pairs):
    """the table cut into the fewest equal chunks of at most LOWER_CHUNK pairs"""
    n = -(-len(pairs) // LOWER_CHUNK)
    size = -(-len(pairs) // n)
    return [pairs[c * size:(c + 1) * size] for c in range(n)]


def lower_chunk_strings(chunk, table):
    """-> (documents `to[i] + to[i+1]`, queries `from[i] + from[i+1]` (cyclic inside the chunk), one query of the runes from +- 1
    that the table `table` does not map)"""
    n = len(chunk)
    docs = [(chr(chunk[i][1]) + chr(chunk[(i + 1) % n][1])).encode() for i in range(n)]
    qs = [(chr(chunk[i][0]) + chr(chunk[(i + 1) % n][0])).encode() for i in range(n)]
    mapped = {a for a, _ in table}
    near = sorted({r for a, _ in chunk for r in (a - 1, a + 1) if r not in mapped and r >= 0x80 and not 0xD800 <= r <= 0xDFFF})
    return docs, qs, "".join(chr(r) for r in near).encode()
