"""The dictionaries and queries of the edit-search tests (tests/test_edit_search_cpu.py, tests/test_gpu_edit_search.py): the smallest
shapes at which the scan, the cut between its two passes and the final rank can go wrong.  tests/test_edit_search_shapes_cpu.py asserts
that they contain the situations their tests are about."""
import numpy as np

import edit_ref as ref

MAX_DISTANCES = (0, 1, 2, 5, 32)
KS = (1, 7, 64, 1024)
SLICES = (1, 2, 7)
ARRAY_SIZES = (1, 64, 65, 257)
CASE_PAIRS = (("K", "k"), ("Ä", "ä"), ("Σ", "σ"), ("Ж", "ж"))     # both members are in the dictionary
LONG70 = "".join(chr(0x430 + i % 32) for i in range(70))


def _word(rng, alphabet, lo, hi):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), int(rng.integers(lo, hi + 1))))


def array_lines(n_docs):
    """empty strings, invalid bytes, 2-, 3- and 4-byte runes, both members of case pairs, a string of 70 runes — then random words
    over a mixed alphabet, cut to n_docs"""
    rng = np.random.default_rng(1234)
    special = [b"", b"\xff\xfe", "été".encode(), "€ 5".encode(), "\U0001f600\U0001f601".encode(), b"", LONG70.encode(),
               b"ab\xf0\x9f\x98", b"\xe2\x82"]
    for up, low in CASE_PAIRS:
        special += [("x" + up).encode(), ("x" + low).encode()]
    alphabet = list("abcXYZ") + ["é", "Ж", "ж", "€", "\U0001f600", "K"]
    lines = special + [_word(rng, alphabet, 0, 9).encode() for _ in range(max(0, n_docs - len(special)))]
    return lines[:n_docs]


DENSE_ALPHABET = "abcD"


def dense_lines():
    """2 048 strings of 1 to 12 runes over four letters: most queries have far more than k matches"""
    rng = np.random.default_rng(77)
    return [_word(rng, DENSE_ALPHABET, 1, 12).encode() for _ in range(2048)]


def _edit(rng, s, alphabet, n):
    s = list(s)
    for _ in range(n):
        op = int(rng.integers(0, 4))
        p = int(rng.integers(0, max(1, len(s))))
        if op == 0 and s:
            del s[p]
        elif op == 1:
            s.insert(p, alphabet[int(rng.integers(0, len(alphabet)))])
        elif op == 2 and s:
            s[p] = alphabet[int(rng.integers(0, len(alphabet)))]
        elif len(s) > 1:
            p = min(p, len(s) - 2)
            s[p], s[p + 1] = s[p + 1], s[p]
    return "".join(s)


def dense_queries(lines):
    """64 queries: the empty one, one rune, exactly 64 runes, 65 runes (flagged), invalid bytes, a dictionary string in the other
    case, then dictionary strings with 0 to 3 edits and random words"""
    rng = np.random.default_rng(78)
    named = [b"", b"c", (DENSE_ALPHABET * 16).encode(), (DENSE_ALPHABET * 16 + "a").encode(), b"\xff\xfe\xff", lines[5].decode().swapcase().encode()]
    out = list(named)
    while len(out) < 64:
        if len(out) % 4 == 3:
            out.append(_word(rng, DENSE_ALPHABET, 1, 14).encode())
        else:
            out.append(_edit(rng, lines[int(rng.integers(0, len(lines)))].decode(), DENSE_ALPHABET, int(rng.integers(0, 4))).encode())
    return out


def chunk_queries(lines):
    """300 queries for the chunked call"""
    rng = np.random.default_rng(79)
    return [_edit(rng, lines[int(rng.integers(0, len(lines)))].decode(), DENSE_ALPHABET, int(rng.integers(0, 3))).encode() for _ in range(300)]


TIE = b"toyota"


def tie_lines():
    """one string 500 times, every other document, between near neighbours: its copies fall in every one of 7 slices"""
    near = [b"toyot", b"toyotas", b"tayota", b"otyota", b"toyoat", b"Toyota", b"toy", b"nissan", b"toyoda", b"oyota"]
    return [TIE if i % 2 == 0 else near[(i // 2) % len(near)] for i in range(1000)]


TIE_QUERIES = [b"toyota", b"toyot", b"tyoota", b"TOYOTA", b"toyotaa", b"nisan"]
TIE_KS = (1, 10, 499)


def transposition_cases():
    """-> (lines, queries): each query an adjacent transposition of a dictionary string, the dictionary sparse enough that a
    transposed string has no other neighbour at distance 1"""
    lines = [b"nissan", b"toyota", b"volkswagen", b"mercedes", b"peugeot", b"hyundai", b"\xd0\xbd\xd0\xb8\xd0\xb2\xd0\xb0", b"ab", b"subaru", b"mitsubishi"]
    queries = []
    for l in lines:
        s = list(l.decode())
        p = next(i for i in range(len(s) - 1) if s[i] != s[i + 1])
        s[p], s[p + 1] = s[p + 1], s[p]
        queries.append("".join(s).encode())
    return lines, queries


def cars_queries(cars_lines, n=200, seed=2024):
    """n of the dictionary's lines with one and two edits applied (Latin letters, so that a typo may hit or miss a q-gram)"""
    rng = np.random.default_rng(seed)
    out = []
    for j, i in enumerate(rng.integers(0, len(cars_lines), n)):
        s = cars_lines[int(i)].decode("utf-8", "replace")
        out.append(_edit(rng, s, "abcdefghijklmnopqrstuvwxyz", 1 + j % 2).encode())
    return out


def rune_pairs(n, seed=5):
    """random pairs of rune strings for the property test of the bounds: short, over small and large alphabets"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        alpha = (3, 8, 70, 5000)[int(rng.integers(0, 4))]
        a = tuple(int(x) for x in rng.integers(0x40, 0x40 + alpha, int(rng.integers(0, 12))))
        b = list(a) if rng.integers(0, 2) else [int(x) for x in rng.integers(0x40, 0x40 + alpha, int(rng.integers(0, 12)))]
        for _ in range(int(rng.integers(0, 4))):                 # a few edits of a copy, among them transpositions
            op, p = int(rng.integers(0, 4)), int(rng.integers(0, max(1, len(b))))
            if op == 0 and b:
                del b[p]
            elif op == 1:
                b.insert(p, int(rng.integers(0x40, 0x40 + alpha)))
            elif op == 2 and b:
                b[p] = int(rng.integers(0x40, 0x40 + alpha))
            elif len(b) > 1:
                p = min(p, len(b) - 2)
                b[p], b[p + 1] = b[p + 1], b[p]
        out.append((a, tuple(b)))
    return out


def runes_of(line, fold):
    return ref.runes(line, fold)


_MEMO = {}


def memo(key, make):
    """a reference computed once per process and shared by the tests that need it (they leave it unchanged)"""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def matrix(name, lines, queries, mode, fold):
    import edit_search_ref as sref
    return memo((name, mode, fold), lambda: sref.distance_matrix(queries, lines, mode, fold))
