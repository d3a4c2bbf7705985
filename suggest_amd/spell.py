"""The spellchecker caller of the fuzzy-search path: pkg/lm's n-gram language model and
pkg/spellchecker.SpellChecker.Predict over the MI355X engine.

  lm = LanguageModel(directory, order=3, start_symbol="<S>", end_symbol="</S>", alphabet=(...))   # Google n-gram files
  sc = SpellChecker(lm)                      # builds + uploads the fuzzy index over the model's vocabulary
  sc.Predict("i am sa", 5, 0.5)              # -> ["sam", ...]            (spellchecker.go:40-92)
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .index import IndexDescription, NGramIndex, _c_desc, _enc, pack_strings

# cmd/spellchecker/cmd/eval.go:16-23
SPELLCHECKER_INDEX = dict(name="words", ngram_size=3, wrap=("^", "$"), pad="$", alphabet=("english", "russian", "numbers", "$^'"))


# save_ngrams(device=None): the writer profiles/lm_store_timing.json shows faster at both sizes timed — the device writer, on
# GPU 0 like from_corpus: 0.011 s against 0.071 s for a 1 M-token model, 0.060 s against 0.261 s for a 4 M-token one
DEFAULT_NGRAM_DEVICE = 0


class LanguageModel:
    """lm.LanguageModel (pkg/lm/language_model.go) loaded from <dir>/{1..order}-gm (pkg/lm/ngram_reader.go)."""

    def __init__(self, directory=None, order=3, start_symbol="<S>", end_symbol="</S>", alphabet=("english", "russian", "numbers", "-."),
                 id_order="lines", binary=None, dictionary=None):
        """directory + id_order: Google count files; "lines" numbers the words by 1-gm line (the reference's test indexer,
        indexer.go:88-114), "count" by (count desc, word asc) like the production build (binary.go:101-199).
        binary + dictionary: RetrieveLMFromBinary (binary.go:59-98) from <name>.lm and <name>.cdb."""
        alpha = (C.c_char_p * len(alphabet))(*[_enc(a) for a in alphabet])
        h = C.c_void_p()
        L = _lib.lib()
        if binary is not None:
            _lib.check(L.sg_lm_load_binary(_enc(binary), _enc(dictionary), _enc(start_symbol), _enc(end_symbol), alpha, len(alphabet), C.byref(h)))
        else:
            _lib.check(L.sg_lm_load_google_ex(_enc(directory), int(order), _enc(start_symbol), _enc(end_symbol), alpha, len(alphabet),
                                              {"lines": 0, "count": 1}[id_order], C.byref(h)))
        self._h = h
        self.order = int(L.sg_lm_order(h))

    def level(self, i):
        """-> (containers u64[], values u64[], total): level i in the reference's packed form (packed_array.go:12-16)"""
        L = _lib.lib()
        nc, nv, tot = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(L.sg_lm_level(self._h, i, None, 0, C.byref(nc), None, 0, C.byref(nv), C.byref(tot)))
        c = np.zeros(nc.value, dtype=np.uint64)
        v = np.zeros(nv.value, dtype=np.uint64)
        _lib.check(L.sg_lm_level(self._h, i, c.ctypes.data, nc.value, C.byref(nc), v.ctypes.data, nv.value, C.byref(nv), C.byref(tot)))
        return c, v, int(tot.value)

    @staticmethod
    def build_files(text, directory, order=3, start_symbol="<S>", end_symbol="</S>", alphabet=("english", "russian", "numbers", "-."),
                    separators=("\n",)):
        """`lm build-lm`: count the k-grams of a corpus into <directory>/{1..order}-gm (pkg/lm/ngram_builder.go, ngram_writer.go)"""
        raw = _enc(text)
        alpha = (C.c_char_p * len(alphabet))(*[_enc(a) for a in alphabet])
        seps = (C.c_char_p * len(separators))(*[_enc(a) for a in separators])
        _lib.check(_lib.lib().sg_lm_build_google(raw, len(raw), int(order), _enc(start_symbol), _enc(end_symbol), alpha, len(alphabet),
                                                 seps, len(separators), _enc(directory)))

    @classmethod
    def from_corpus(cls, text, order=3, start_symbol="<S>", end_symbol="</S>", alphabet=("english", "russian", "numbers", "-."),
                    separators=("\n",), id_order="count", device=0):
        """The model of a corpus, built on the GPU (sg_lm_build_device): what build_files + LanguageModel(directory, id_order=...)
        give, with no files in between.  id_order "count": (count desc, word asc), the production numbering; "lines": first
        appearance, the line order build_files writes."""
        raw = text if isinstance(text, (bytes, bytearray, memoryview)) else _enc(text)
        buf = np.frombuffer(raw, dtype=np.uint8)
        alpha = (C.c_char_p * len(alphabet))(*[_enc(a) for a in alphabet])
        seps = (C.c_char_p * len(separators))(*[_enc(a) for a in separators])
        h = C.c_void_p()
        L = _lib.lib()
        _lib.check(L.sg_lm_build_device(buf.ctypes.data if buf.size else None, buf.size, int(order), _enc(start_symbol), _enc(end_symbol),
                                        alpha, len(alphabet), seps, len(separators), {"lines": 0, "count": 1}[id_order], int(device), C.byref(h)))
        self = cls.__new__(cls)
        self._h = h
        self.order = int(L.sg_lm_order(h))
        return self

    def save(self, binary, dictionary, mph=False):
        """Write the model as <binary> (.lm, nGramModel.Store) and <dictionary> (.cdb, BuildCDBDictionary): the pair
        LanguageModel(binary=..., dictionary=...) loads.  mph=True appends the minimal perfect hash the reference's
        RetrieveLMFromBinary reads after the model (sg_lm_store_binary_ex with SG_LM_STORE_MPH): the file Go opens."""
        _lib.check(_lib.lib().sg_lm_store_binary_ex(self._h, _enc(binary), _enc(dictionary), _lib.SG_LM_STORE_MPH if mph else 0))

    def save_ngrams(self, directory, device=None):
        """Write the model as Google n-gram files <directory>/{1..order}-gm (sg_lm_store_google): what the reference's build-lm
        step reads, and what LanguageModel(directory, id_order="lines") loads back array for array.  device >= 0 formats the
        lines on that GPU, -1 runs the host writer; both write identical files.  None: GPU 0 — the device writer is 4 to 6 times
        faster than the host writer at both sizes timed (profiles/lm_store_timing.json); without a GPU pass -1."""
        dev = DEFAULT_NGRAM_DEVICE if device is None else int(device)
        _lib.check(_lib.lib().sg_lm_store_google(self._h, _enc(os.fspath(directory)), dev))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().sg_lm_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(_lib.lib().sg_lm_num_words(self._h))

    def word(self, i):
        buf = C.create_string_buffer(256)
        n = _lib.lib().sg_lm_word(self._h, int(i), buf, 256)
        if n > 256:
            buf = C.create_string_buffer(n)
            _lib.lib().sg_lm_word(self._h, int(i), buf, n)
        return buf.raw[:n]

    def words(self):
        return [self.word(i) for i in range(len(self))]

    def GetWordID(self, token):                                # indexer.go:50-63 (0xFFFFFFFF = unknown)
        t = _enc(token)
        return int(_lib.lib().sg_lm_word_id(self._h, t, len(t)))

    def _ids(self, words):
        return np.array([self.GetWordID(w) for w in words], dtype=np.uint32)

    def Score(self, words):                                    # NGramModel.Score
        ids = self._ids(words)
        return float(_lib.lib().sg_lm_score(self._h, ids.ctypes.data, len(ids)))

    def ScoreSentence(self, words):                            # LanguageModel.ScoreSentence
        ids = self._ids(words)
        return float(_lib.lib().sg_lm_score_word_ids(self._h, ids.ctypes.data, len(ids)))

    def _vocab(self):
        """token bytes -> word id, built once (Indexer.Get without a call per token; a word listed twice keeps its first id)"""
        v = getattr(self, "_vocab_ids", None)
        if v is None:
            v = {}
            for i, w in enumerate(self.words()):
                v.setdefault(w, i)
            self._vocab_ids = v
        return v

    def ScoreSentenceBatch(self, sentences, device=0):
        """ScoreSentence for every token list of `sentences` on the GPU (sg_lm_score_word_ids_batch) -> float64 [n]"""
        v = self._vocab()
        lens = np.array([len(s) for s in sentences], dtype=np.uint64)
        offs = np.zeros(len(sentences) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens, dtype=np.uint64)
        ids = np.fromiter((v.get(_enc(w), 0xFFFFFFFF) for s in sentences for w in s), dtype=np.uint32, count=int(offs[-1]))
        return self.score_word_ids_batch(ids, offs, device)

    def score_word_ids_batch(self, ids, offs, device=0):
        """ScoreWordIDs of ids[offs[i] .. offs[i+1]) for every i on the GPU -> float64 [n]"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        out = np.zeros(n, dtype=np.float64)
        _lib.check(_lib.lib().sg_lm_score_word_ids_batch(self._h, int(device), ids.ctypes.data if ids.size else None, offs.ctypes.data, n,
                                                         out.ctypes.data))
        return out

    def score_text_batch(self, lines=None, blob=None, offs=None, device=0):
        """`lm eval` for a batch: ScoreSentence(Tokenize(line)) of every line on the GPU (sg_lm_score_text_batch)
        -> (scores float64 [n], words uint32 [n] = len(Tokenize(line)), unknown uint32 [n] = its tokens without an id)"""
        if blob is None:
            blob, offs = pack_strings(lines)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        scores = np.zeros(n, dtype=np.float64)
        words = np.zeros(n, dtype=np.uint32)
        unknown = np.zeros(n, dtype=np.uint32)
        _lib.check(_lib.lib().sg_lm_score_text_batch(self._h, int(device), blob.ctypes.data if blob.size else None, offs.ctypes.data, n,
                                                     scores.ctypes.data, words.ctypes.data, unknown.ctypes.data))
        return scores, words, unknown

    def score_text_batch_device(self, d_blob, d_offs, n, text_bytes, d_scores, d_words=None, d_unknown=None, stream=0, device=0):
        """sg_lm_score_text_batch_device: raw device pointers (torch tensors' data_ptr()), asynchronous on `stream`"""
        _lib.check(_lib.lib().sg_lm_score_text_batch_device(self._h, int(device), d_blob, d_offs, int(n), int(text_bytes), d_scores, d_words,
                                                            d_unknown, stream))

    def next_score(self, context, word, model_level=False):
        """Next(context).ScoreNext(word) -> (status, score); status 0 scorer, 1 nil scorer, 2 error"""
        ids = self._ids(context)
        v = C.c_double(0)
        st = _lib.lib().sg_lm_next_score(self._h, ids.ctypes.data, len(ids), self.GetWordID(word), 1 if model_level else 0, C.byref(v))
        return int(st), float(v.value)

    def Tokenize(self, text):                                  # lm.NewTokenizer(alphabet).Tokenize
        raw = _enc(text)
        buf = C.create_string_buffer(len(raw) * 3 + 64)            # (an invalid byte is U+FFFD, three bytes, when that is a letter)
        n = _lib.lib().sg_lm_tokenize(self._h, raw, len(raw), buf, len(buf))
        return buf.value.split(b"\n") if n else []


class SpellChecker:
    """spellchecker.SpellChecker (pkg/spellchecker/spellchecker.go:14-37) wired like
    internal/spellchecker/dep/spellchecker.go:14-53: fuzzy index over the model's vocabulary, docID = word id."""

    def __init__(self, model, description=None, device=0):
        self.model = model
        self.description = description or IndexDescription(**SPELLCHECKER_INDEX)
        desc = _c_desc(self.description)
        h = C.c_void_p()
        _lib.check(_lib.lib().sg_spell_index_build(model._h, C.byref(desc), int(device), C.byref(h)))
        self.index = NGramIndex(description=self.description, device=device, upload=False, _handle=h)
        self.index.device = int(device)

    def predict_batch(self, queries=None, top_k=5, similarity=0.5, blob=None, offs=None):
        """-> (ids uint32 [n, top_k + 1], counts uint32 [n]) — word ids of the predictions, best first"""
        if blob is None:
            blob, offs = pack_strings(queries)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        ids = np.zeros((n, int(top_k) + 1), dtype=np.uint32)
        cnt = np.zeros(n, dtype=np.uint32)
        _lib.check(_lib.lib().sg_spell_predict_batch(self.index._h, self.model._h, blob.ctypes.data if blob.size else None, offs.ctypes.data,
                                                     n, int(top_k), float(similarity), ids.ctypes.data, cnt.ctypes.data))
        return ids, cnt

    def predict_batch_device(self, d_blob, d_offs, n_q, q_bytes, top_k, similarity, d_ids, d_counts, stream=0):
        """sg_spell_predict_batch_device: raw device pointers (torch tensors' data_ptr()), asynchronous on `stream`"""
        _lib.check(_lib.lib().sg_spell_predict_batch_device(self.index._h, self.model._h, d_blob, d_offs, int(n_q), int(q_bytes), int(top_k),
                                                            float(similarity), d_ids, d_counts, stream))

    def Predict(self, query, topK, similarity):
        ids, cnt = self.predict_batch([query], topK, similarity)
        c = int(cnt[0])
        if c == _lib.SG_COUNT_REF_PANIC:
            raise RuntimeError("reference behaviour: panic: makechan: size out of range (suggester.go:62)")
        if c == _lib.SG_COUNT_REF_DEADLOCK:
            raise RuntimeError("reference behaviour: deadlock (suggester.go:62)")
        if c == _lib.SG_COUNT_LM_ERROR:
            raise ValueError("nGrams length should be less than the nGramModel order")
        if c == _lib.SG_COUNT_TOO_LONG:
            raise ValueError("query word has more than SG_MAX_QUERY_TERMS n-grams")
        return [self.model.word(int(i)).decode("utf-8", "replace") for i in ids[0, :c]]
