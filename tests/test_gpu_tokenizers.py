"""The device tokenisers over the description space (tests/tokenizer_shapes.py) against the CPU oracle: d_tokenize's three bodies
(ASCII in registers, general, sequential decode) from the fused kernel, sg_terms_kernel, plan_one_query, build_tokenize and
build_tokenize_long, sg_plan2_kernel's half-wavefront copy and long_tokenize — under fifteen descriptions, every launch that
reaches one of them, bit for bit: ids, order, score bits, counts (pkg/suggest/tokenizer.go:9-34, pkg/analysis, pkg/alphabet).
tests/test_tokenizer_shapes_cpu.py holds the inputs to the edges these cases are about."""
import numpy as np
import pytest

import oracle
import tokenizer_shapes as ts
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

CALLS = (("jaccard", 0.3, 10), ("cosine", 0.6, 5), ("overlap", 0.5, 70), ("exact", 1.0, 3))
DEFAULTS = dict(SG_PIPE=2, SG_PRETOK=2048, SG_PLAN2=1, SG_TIGHTEN=2, SG_ORDER=1)
# name -> (knobs, takes the pipeline, the batch in the interleaved order)
LAUNCHES = {
    "fused": (dict(SG_PIPE=0, SG_PRETOK=0), False, False),
    "fused-pretok": (dict(SG_PIPE=0, SG_PRETOK=1), False, False),
    "pipe-plan": (dict(SG_PIPE=1, SG_PLAN2=0, SG_PRETOK=1, SG_TIGHTEN=0), True, False),
    # (SG_ORDER=1 orders batches of 8 192 queries and more: this batch keeps its own order; SG_ORDER=2 has the order kernels
    #  sort it, heaviest first, and sg_plan2_kernel reads its queries through that list)
    "pipe-plan2-natural": (dict(SG_PIPE=1, SG_PLAN2=1, SG_PRETOK=1, SG_TIGHTEN=0, SG_ORDER=1), True, False),
    "pipe-plan2-ordered": (dict(SG_PIPE=1, SG_PLAN2=1, SG_PRETOK=1, SG_TIGHTEN=0, SG_ORDER=2), True, False),
    "pipe-plan2-interleaved": (dict(SG_PIPE=1, SG_PLAN2=1, SG_PRETOK=1, SG_TIGHTEN=0, SG_ORDER=0), True, True),
}


class _Case:
    def __init__(self, name):
        from suggest_amd import IndexDescription, NGramIndex
        self.name, self.desc = name, ts.description(name)
        self.docs, self.queries = ts.dictionary(self.desc), ts.queries(self.desc)
        self.gpu = NGramIndex(self.docs, IndexDescription(**self.desc))
        self.ora = oracle.OracleIndex(self.docs, **self.desc)
        self.packed = oracle.pack_strings(self.queries)
        self.order = np.array(ts.interleaved(self.desc, self.queries))
        self.shuffled = [self.queries[i] for i in self.order]
        self.packed_shuffled = oracle.pack_strings(self.shuffled)
        self._want = {}

    def want(self, call):
        """the oracle's rows of a call, computed once and left alone"""
        if call not in self._want:
            rows = self.ora.suggest_batch(*self.packed, *call)[:3]
            for a in rows:
                a.setflags(write=False)
            self._want[call] = rows
        return self._want[call]


@pytest.fixture(scope="module", params=ts.NAMES)
def case(request):
    c = _Case(request.param)
    yield c
    c.gpu.close()


def _worth_comparing(counts, name):
    flagged, share = ts.filled(counts)
    assert flagged == 0 and share >= 0.9, (name, flagged, share)


@pytest.mark.parametrize("call", CALLS, ids=lambda c: "%s-%g-k%d" % c)
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_rows_are_the_oracles(case, launch, call):
    knobs, pipeline, shuffled = LAUNCHES[launch]
    qb, qo = case.packed_shuffled if shuffled else case.packed
    qs = case.shuffled if shuffled else case.queries
    want = case.want(call)
    if shuffled:
        want = tuple(a[case.order] for a in want)
    try:
        case.gpu.tune(**knobs)
        before = case.gpu.pipe_stats()["queries"]
        got = case.gpu.suggest_batch(blob=qb, offs=qo, metric=call[0], similarity=call[1], k=call[2])
        grew = case.gpu.pipe_stats()["queries"] - before
    finally:
        case.gpu.tune(**DEFAULTS)
    assert_same(got, want, qs)
    assert grew == (len(qs) if pipeline else 0), (case.name, launch, call)      # the launch ran the path it is here for
    if call == CALLS[0]:
        _worth_comparing(got[2], case.name)                  # (a comparison of empty rows proves nothing)


def test_autocomplete_is_the_oracles(case):
    """no closing wrap: another byte length under the guard of ngram_tokenizer.go:18, another end to trim"""
    pre = ts.prefixes()
    pb, po = oracle.pack_strings(pre)
    for limit in (7, 80):
        ids, cnt = case.gpu.autocomplete_batch(blob=pb, offs=po, limit=limit)
        oi, oc, _ = case.ora.autocomplete_batch(pb, po, limit)
        bad = np.nonzero(cnt != oc)[0]
        assert bad.size == 0, (case.name, limit, [pre[i] for i in bad[:5]], cnt[bad[:5]], oc[bad[:5]])
        valid = (np.arange(limit)[None, :] < np.minimum(oc, limit)[:, None]) & (oc < ts.SPECIAL)[:, None]
        rows = np.nonzero((valid & (ids != oi)).any(axis=1))[0]
        assert rows.size == 0, (case.name, limit, [pre[i] for i in rows[:5]])


def test_device_build_is_the_host_build(case):
    """build_tokenize, and build_tokenize_long for the documents above 128 n-grams"""
    from suggest_amd import IndexDescription, NGramIndex
    desc = IndexDescription(**case.desc)
    host = NGramIndex(case.docs, desc, upload=False)
    dev = NGramIndex(case.docs, desc, upload=False, build="device")
    try:
        assert dev.stats() == host.stats(), case.name
        assert dev.digest() == host.digest(), case.name
        dev.upload()
        call = CALLS[0]
        assert_same(dev.suggest_batch(blob=case.packed[0], offs=case.packed[1], metric=call[0], similarity=call[1], k=call[2]), case.want(call), case.queries)
    finally:
        host.close()
        dev.close()


def test_descriptions_over_the_term_key_are_refused():
    """q x pad runes above the key's eight symbols: the device packer has no overflow guard of its own and relies on this refusal"""
    from suggest_amd import IndexDescription, NGramIndex
    assert [d["ngram_size"] * len(d["pad"]) for d in ts.OVER_THE_KEY] == [9, 10]
    for d in ts.OVER_THE_KEY:
        for build in ("host", "device"):
            with pytest.raises(Exception, match="8-symbol term key"):
                NGramIndex([ts.FIRST_DOC, b"abc$", "é_é".encode()], IndexDescription(**d), upload=False, build=build)
