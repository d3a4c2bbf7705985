"""Every pair of the lower-case table (suggest_amd/csrc/unicode_lower.inc, 1 364 {from, to}) through d_lower, the device's
unicode.ToLower (strings.ToLower of pkg/analysis/filter_tokenizer.go:21): an index over the `to` runes, queried with the `from`
runes, against the oracle — whose table is generated from another source (tests/test_tokenizer_shapes_cpu.py holds the two
files to one another).  q = 1 and no wrap: a token per distinct rune, so a rune that is mapped wrongly, or not at all, is a pad."""
import os

import pytest

import oracle
import tokenizer_shapes as ts
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

PAIRS = ts.lower_pairs(os.path.join(oracle.ROOT, "suggest_amd", "csrc", "unicode_lower.inc"))
CHUNKS = ts.lower_chunks(PAIRS)           # (tests/test_tokenizer_shapes_cpu.py: they cover the table)
DEFAULTS = dict(SG_PIPE=2, SG_PRETOK=2048)
LAUNCHES = (dict(SG_PIPE=0, SG_PRETOK=0), dict(SG_PIPE=0, SG_PRETOK=1))     # the fused kernel tokenising itself; behind sg_terms_kernel


@pytest.mark.parametrize("c", range(len(CHUNKS)))
def test_every_pair_goes_through_d_lower(c):
    from suggest_amd import IndexDescription, NGramIndex
    pairs = CHUNKS[c]
    docs, qs, near = ts.lower_chunk_strings(pairs, PAIRS)
    desc = dict(ngram_size=1, wrap=("", ""), pad="$", alphabet=("".join(sorted({chr(b) for _, b in pairs})),))
    gpu = NGramIndex(docs, IndexDescription(**desc))
    ora = oracle.OracleIndex(docs, **desc)
    qb, qo = oracle.pack_strings(qs + [near])
    try:
        for knobs in LAUNCHES:
            gpu.tune(**knobs)
            for metric, alpha, k in (("exact", 1.0, 1), ("jaccard", 0.5, 5)):
                got = gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k)
                assert_same(got, ora.suggest_batch(qb, qo, metric, alpha, k), qs + [near])
                ids, sc, cnt = got
                assert (cnt[:len(qs)] >= 1).all() and (sc[:len(qs), 0] == 1.0).all()
                wrong = [hex(pairs[i][0]) for i in range(len(qs)) if docs[int(ids[i, 0])] != docs[i]]
                assert not wrong, wrong
    finally:
        gpu.tune(**DEFAULTS)
        gpu.close()
    # the `from` strings as documents: build_tokenize lower-cases them like the host builder
    host = NGramIndex(qs, IndexDescription(**desc), upload=False)
    dev = NGramIndex(qs, IndexDescription(**desc), upload=False, build="device")
    assert dev.stats() == host.stats() and dev.digest() == host.digest()
