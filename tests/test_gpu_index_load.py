"""sg_index_load_reference_ex with the device decoder (index_load.inc): the index it assembles against the host reader's word
for word and against refindex.read_index list by list, round trips through the device encoder, searches after a device-decoded
load, the malformed lists of index_load_shapes.py refused as the host reader refuses them, and the search path left alone."""
import os

import numpy as np
import pytest

import refindex
from conftest import CARS_DESC, WORDS_DESC
from index_load_shapes import (FOREIGN_DESC, MALFORMED_TERM, SG_E_INVALID, assert_same_index, foreign_files, malformed_files, malformed_lists,
                               no_terms_files, pair_twice_files)
from index_store_shapes import SHAPES_DESC, dropped_repeats_files, shapes_files

pytestmark = pytest.mark.gpu


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(**d)


def _both(hd, dl, desc):
    from suggest_amd import NGramIndex
    dev = NGramIndex.from_reference_files(hd, dl, desc, upload=False, decode_device=0)
    host = NGramIndex.from_reference_files(hd, dl, desc, upload=False)
    assert_same_index(dev, host)
    return dev


def _without_repeats(lists):
    return {k: (raw, [x for i, x in enumerate(post) if i == 0 or x != post[i - 1]]) for k, (raw, post) in lists.items()}


@pytest.mark.parametrize("name, desc", [("cars", CARS_DESC), ("words_subset", WORDS_DESC)])
def test_fixture_decoded_on_the_device(name, desc, golden_dir):
    hd, dl = os.path.join(golden_dir, "db", name + ".hd"), os.path.join(golden_dir, "db", name + ".dl")
    dev = _both(hd, dl, _desc(desc))
    _, ref = refindex.read_index(hd, dl)
    if name == "words_subset":
        assert sum(1 for raw, _ in ref.values() if raw > 256) == 40
    assert dev.lists() == _without_repeats(ref)


def test_edge_shapes_decoded_on_the_device(tmp_path, golden_dir):
    lists, names, hd, dl = shapes_files(tmp_path, golden_dir)
    got = _both(hd, dl, _desc(SHAPES_DESC)).lists()
    _, ref = refindex.read_index(hd, dl)
    want = _without_repeats(ref)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], names[k]


def test_dropped_repeats_decoded_on_the_device(tmp_path, golden_dir):
    desc, hd, dl = dropped_repeats_files(tmp_path, golden_dir)
    got = _both(hd, dl, _desc(desc)).lists()
    _, ref = refindex.read_index(hd, dl)
    assert got == _without_repeats(ref)
    assert any(raw > 256 and raw > len(post) for raw, post in got.values())


def test_foreign_lists_decoded_on_the_device(tmp_path, golden_dir):
    hd, dl, want = foreign_files(tmp_path, golden_dir)
    assert {k: v[1] for k, v in _both(hd, dl, _desc(FOREIGN_DESC)).lists().items()} == want
    hd, dl = no_terms_files(tmp_path, golden_dir)
    assert _both(hd, dl, _desc(FOREIGN_DESC)).lists() == {}


def test_pair_with_two_lists_takes_the_host_decoders(tmp_path, golden_dir):
    hd, dl, want = pair_twice_files(tmp_path, golden_dir)
    assert _both(hd, dl, _desc(FOREIGN_DESC)).lists() == want


def test_two_loads_give_the_same_arrays(golden_dir):
    from suggest_amd import NGramIndex
    hd, dl = os.path.join(golden_dir, "db", "words_subset.hd"), os.path.join(golden_dir, "db", "words_subset.dl")
    a, b = (NGramIndex.from_reference_files(hd, dl, _desc(WORDS_DESC), upload=False, decode_device=0) for _ in range(2))
    assert_same_index(a, b)


def _round_trip(lines, desc, tmp_path):
    """built on the device, saved with the device encoder, loaded with the device decoder"""
    from suggest_amd import NGramIndex
    built = NGramIndex(lines, _desc(desc), device=0, upload=False, build="device")
    hd, dl = str(tmp_path / "rt.hd"), str(tmp_path / "rt.dl")
    built.save(hd, dl, device=0)
    dev = _both(hd, dl, _desc(desc))
    # a save orders the terms by segment, then as sg_index_lists gives them: the term numbering of a loaded
    # index, and with it its digest, is the files' — the lists, the counters and the host-loaded copy are the comparison
    assert dev.lists() == built.lists()
    sa, sb = dev.stats(), built.stats()
    for key in ("n_docs", "n_segments", "n_terms", "n_lists", "n_postings", "n_postings_raw", "posting_bytes"):
        assert sa[key] == sb[key], key
    return dev


def test_cars_round_trip(cars_lines, tmp_path):
    _round_trip(cars_lines, CARS_DESC, tmp_path)


def test_words_round_trip(words_lines, tmp_path):
    dev = _round_trip(words_lines, WORDS_DESC, tmp_path)
    raws = [raw for raw, _ in dev.lists().values()]
    assert min(sum(1 for r in raws if r <= 65), sum(1 for r in raws if 65 < r <= 256), sum(1 for r in raws if r > 256)) > 1000


def _queries(cars_lines, n):
    from suggest_amd import pack_strings
    queries = [l[:-1] if i % 3 == 0 and len(l) > 4 else l for i, l in enumerate(cars_lines[::(len(cars_lines) // n)][:n])]
    assert len(queries) == n
    return pack_strings(queries)


def _rows(index, qb, qo):
    out = []
    for metric, alpha, k in (("jaccard", 0.5, 10), ("cosine", 0.4, 20)):
        out.extend(index.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k))
    out.extend(index.autocomplete_batch(blob=qb, offs=qo, limit=10))
    return out


def _same_rows(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))     # ids, score bits, counts


def test_search_after_a_device_decoded_load(cars_lines, golden_dir):
    from suggest_amd import NGramIndex
    hd, dl = os.path.join(golden_dir, "db", "cars.hd"), os.path.join(golden_dir, "db", "cars.dl")
    qb, qo = _queries(cars_lines, 300)
    host = _rows(NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), device=0), qb, qo)
    assert int(host[2].sum()) > 0
    _same_rows(_rows(NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), device=0, decode_device=0), qb, qo), host)


def test_load_leaves_the_search_path_alone(cars_lines, golden_dir):
    from suggest_amd import NGramIndex
    qb, qo = _queries(cars_lines, 200)
    ix = NGramIndex(cars_lines, _desc(CARS_DESC), device=0)
    before = _rows(ix, qb, qo)
    assert int(before[2].sum()) > 0
    hd, dl = os.path.join(golden_dir, "db", "words_subset.hd"), os.path.join(golden_dir, "db", "words_subset.dl")
    other = NGramIndex.from_reference_files(hd, dl, _desc(WORDS_DESC), upload=False, decode_device=0)
    _same_rows(_rows(ix, qb, qo), before)
    assert ix.replicas() == [0] and other.replicas() == []


@pytest.mark.parametrize("name", sorted(malformed_lists()))
def test_malformed_list_is_refused(name, tmp_path, golden_dir):
    from suggest_amd import NGramIndex, _lib
    hd, dl = malformed_files(tmp_path, golden_dir, name)
    seen = []
    for decode_device in (None, 0):
        with pytest.raises(_lib.SuggestHipError) as e:
            NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), upload=False, decode_device=decode_device)
        assert e.value.code == SG_E_INVALID
        assert "'%s'" % MALFORMED_TERM.decode() in str(e.value)
        seen.append(str(e.value))
    assert seen[0] == seen[1]
