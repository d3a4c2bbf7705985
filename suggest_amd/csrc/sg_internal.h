// sg_internal.h — structures shared by the host index builder (host_index.cpp) and the
// HIP engine (engine.hip).  Not part of the public ABI (include/suggest_hip.h).
#pragma once

#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/suggest_hip.h"

namespace sg {

constexpr uint32_t kNoTerm = 0xFFFFFFFFu;
constexpr uint32_t kRuneError = 0xFFFD;

// Symbol table: every rune that can appear in a normalised term (alphabet runes + the runes of
// the pad string) gets an id 1..255; a term is at most 8 symbols and is packed little-endian
// into a u64 (byte i = symbol i, 0 = end).  Key equality == reference term-string equality.
struct Symbols {
  uint8_t ascii_sym[128];    // symbol id of an ASCII rune, 0 = not a symbol
  uint8_t ascii_alpha[128];  // 1 = Alphabet.Has(rune)
  std::vector<uint32_t> na_rune;  // non-ASCII symbol runes, ascending
  std::vector<uint8_t> na_sym, na_alpha;
  uint8_t pad_sym[8];
  uint32_t n_pad = 0;
  std::vector<uint32_t> sym_rune;  // id -> rune (index 0 unused)
};

struct TermSlot {  // open-addressing hash table slot (16 B)
  uint64_t key;
  uint32_t term;  // kNoTerm = empty
  uint32_t pad;
};

struct DupEntry {  // a (term, segment, doc) whose doc repeats the term
  uint32_t term, segment, doc, mult;
};

struct HostIndex {
  // description
  uint32_t q = 3;
  std::vector<uint32_t> wrap0, wrap1;  // runes
  std::string wrap0_s, wrap1_s, pad_s;
  std::vector<std::string> alphabet_spec;
  Symbols sym;

  uint64_t n_docs = 0;
  uint32_t n_segments = 0;  // == header.Indices of the reference (max cardinality + 1)
  uint32_t min_segments = 0;  // builders: at least this many segments (docID-sharded indexes agree on the global number)
  std::vector<uint64_t> term_key;                    // termID -> key
  std::unordered_map<uint64_t, uint32_t> term_of;    // key -> termID
  std::vector<uint32_t> seg_off;                     // [n_terms*(S+1)] chunk (16 B) offsets, term-major
  std::vector<uint32_t> list_len;                    // [n_terms*S] stored (de-duplicated) lengths
  std::vector<uint32_t> postings;                    // padded chunks, ascending docIDs per (term, segment)
  std::vector<DupEntry> dups;                        // docs with repeated terms, ascending (term, segment, doc)
  std::vector<TermSlot> slots;                       // hash table, size = power of two
  uint64_t n_lists = 0, n_postings = 0, n_postings_raw = 0;
};

// host tokenizer (NewSuggestTokenizer / NewAutocompleteTokenizer, pkg/suggest/tokenizer.go:9-34)
// -> packed term keys, repeats included, first-occurrence order.  Returns false if a term does
// not fit the 8-symbol key.
bool tokenize_keys(const HostIndex& ix, const uint8_t* s, size_t n, bool autocomplete, std::vector<uint64_t>& out);

int build_host_index(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, HostIndex& ix,
                     std::string& err);

int init_description(const sg_desc* desc, HostIndex& ix, std::string& err);
bool term_string_key(const HostIndex& ix, const std::string& term, uint64_t* key);
void build_term_table(HostIndex& ix);
// loads reference-built <name>.hd / <name>.dl (ref_index_reader.cpp); seconds (may be null): [4] file read, header parse and
// term interning, list decode, assembly
int load_reference_index(const char* hd_path, const char* dl_path, const sg_desc* desc, HostIndex& ix, std::string& err, double* seconds = nullptr);
// ---- its three steps, shared with the device decoder (index_load.inc) ----
struct RefTerm { std::string term; uint32_t indice = 0, size = 0, pos = 0, len = 0; };   // a termDescription of the header
struct RefList {     // a descriptor that passed the checks of step 1: size != 0, indice < Indices, pos + size inside the .dl, the alphabet
  uint32_t term, segment;
  uint32_t raw;      // PostingListLen: picks the codec
  uint32_t size, pos;
  uint32_t desc;     // its RefTerm (the error messages name the term)
};
struct RefFiles {
  std::vector<uint8_t> dl;
  std::vector<RefTerm> terms;
  std::vector<RefList> lists;          // header order; up to the first descriptor that was refused
  int fail_rc = 0;                     // that refusal: returned unless a list before it is malformed (the order the errors are met in)
  std::string fail_err;
};
// 1: read, parse, intern, check; seconds (may be null): [2] file read, the rest
int ref_open(const char* hd_path, const char* dl_path, const sg_desc* desc, HostIndex& ix, RefFiles& f, std::string& err, double seconds[2]);
// 2 + 3 on the host; seconds (may be null): [2] decode, assembly
int ref_decode_host(HostIndex& ix, const RefFiles& f, std::string& err, double seconds[2]);
bool ref_pair_twice(const HostIndex& ix, const RefFiles& f);
bool ref_decode_list(const RefFiles& f, const RefList& l, std::vector<uint32_t>& out);            // false: malformed (or empty)
int ref_malformed(const RefFiles& f, const RefList& l, std::string& err);                        // the message; -> SG_E_INVALID
void ref_dedup(HostIndex& ix, const RefList& l, std::vector<uint32_t>& v);                       // v de-duplicated, ix.dups appended to
void ref_marker(HostIndex& ix, const RefList& l, size_t stored);                                 // raw > 256 > stored: the marker entry
int ref_layout(HostIndex& ix, const RefFiles& f, const uint32_t* stored, std::string& err);      // list_len, counters, seg_off, postings zeroed
void ref_put_list(HostIndex& ix, const RefList& l, const std::vector<uint32_t>& v);              // a list into its chunks, the last one padded
void ref_finish(HostIndex& ix);                                                                  // dups sorted, the term table

// ---- saving an index as reference-format <name>.hd / <name>.dl (index_store.cpp; the device encoder: index_store.inc) ----
struct StoreList {   // one non-empty (segment, term) list; the header order is segment ascending, then the order of sg_index_lists
  uint64_t src;      // its first posting in HostIndex::postings
  uint32_t term, segment;
  uint32_t len;      // stored (de-duplicated) length
  uint32_t raw;      // PostingListLen: with the repeats of `dups` (and of a marker entry, doc == 0xFFFFFFFF) — picks the codec
  uint32_t dup_begin, dup_n;   // dups[dup_begin .. dup_begin + dup_n): this list's repeats, the marker entry left out
};
int store_lists(const HostIndex& ix, std::vector<StoreList>& out, std::string& err);
// the plain host encoder: size[i] bytes of list i, back to back in `dl`
void store_encode_host(const HostIndex& ix, const std::vector<StoreList>& lists, std::vector<uint32_t>& size, std::vector<uint8_t>& dl);
// exclusive scan of the sizes in header order; SG_E_UNSUPPORTED where the .dl would reach 4 GiB (PostingListPosition is a uint32)
int store_positions(const std::vector<uint32_t>& size, std::vector<uint32_t>& pos, uint64_t* total, std::string& err);
// writes the .dl bytes and the gob header; seconds[0] = the header's share of the time (null: not wanted)
int store_write_files(const HostIndex& ix, const std::vector<StoreList>& lists, const std::vector<uint32_t>& size,
                      const std::vector<uint32_t>& pos, const uint8_t* dl, uint64_t dl_bytes, const char* hd_path, const char* dl_path,
                      double* header_seconds, std::string& err);
// D. J. Bernstein's constant database with key = record number as 4 bytes little endian (dictionary.BuildCDBDictionary,
// pkg/dictionary/helpers.go:52-95): value(i, &len) = the bytes of record i
int cdb_write_dictionary(const char* path, size_t n, const std::function<const char*(size_t, size_t*)>& value, std::string& err);
// ... and its reader (dictionary.OpenCDBDictionary; lm.cpp): the values in record-number order.  false: the file cannot be opened,
// is truncated or corrupted, or its record numbers have a hole (err says which).  lm_load_binary and sg_dictionary_open_cdb use it.
bool read_cdb_words(const char* path, std::vector<std::string>& words, std::string& err);

// metric maths in IEEE double, evaluation order of pkg/metric/*.go (host copies; engine.hip has
// the device twins)
int metric_min_y(int m, double alpha, int size);
int metric_max_y(int m, double alpha, int size);
int metric_threshold(int m, double alpha, int a, int b);

uint64_t mix64(uint64_t k);

uint32_t host_next_rune(const uint8_t* s, size_t n, size_t* adv);   // Go range decoding (invalid byte -> U+FFFD, width 1)
uint32_t host_lower_rune(uint32_t r);                                // unicode.ToLower (simple mappings)
uint32_t host_utf8_width(uint32_t r);
bool host_alphabet_has(const std::vector<std::string>& spec, uint32_t r);   // alphabet.CreateAlphabet(spec).Has(r)
void host_alphabet_runes(const std::vector<std::string>& spec, std::vector<uint32_t>& out);   // every rune it has, ascending

// ---- language model of the spellchecker caller (lm.cpp) ----
constexpr uint32_t kUnknownWord = 0xFFFFFFFFu;      // pkg/lm/indexer.go:16
constexpr uint32_t kNoContext = 0xFFFFFFFDu;        // InvalidContextOffset, pkg/lm/ngram_vector.go:25-27

struct LmLevel {   // n-grams of one order, sorted by (parent, word); the index of an entry is its "context offset"
  std::vector<uint32_t> word, count;
  std::vector<uint32_t> child_begin;   // [n_parents + 2]: entries whose parent is p are child_begin[p] .. child_begin[p + 1];
                                       // the last bucket (p = n_parents) holds entries without a parent (kNoContext)
  uint64_t total = 0;                  // CorpusCount
};

struct HostLM {
  std::vector<std::string> words;      // id order (lines of 1-gm)
  std::unordered_map<std::string, uint32_t> id_of;
  std::vector<LmLevel> level;          // order 1 .. N
  uint32_t order = 0, start_symbol = kUnknownWord, end_symbol = kUnknownWord;
  std::vector<std::string> alphabet;
};

struct LmNext {    // NGramModel.Next: the continuations of a context = one bucket of one level
  int status = 0;  // 0 scorer, 1 nil scorer, 2 error (pkg/lm/ngram_model.go:64-98)
  uint32_t level = 0, from = 0, to = 0;
  uint32_t context_count = 0;          // count of the context itself (the denominator of ScoreNext)
};

int lm_load_google(const char* dir, uint32_t order, const char* start_symbol, const char* end_symbol, const std::vector<std::string>& alphabet,
                   int id_order, HostLM& lm, std::string& err);
int lm_load_binary(const char* lm_path, const char* cdb_path, const char* start_symbol, const char* end_symbol,
                   const std::vector<std::string>& alphabet, HostLM& lm, std::string& err);
int lm_store_binary(const HostLM& lm, const char* lm_path, const char* cdb_path, uint32_t flags, std::string& err);   // flags: SG_LM_STORE_*
void lm_level_packed(const HostLM& lm, uint32_t level, std::vector<uint64_t>& containers, std::vector<uint64_t>& values, uint32_t* total);
int lm_build_google_files(const uint8_t* text, size_t n, uint32_t order, const char* start_symbol, const char* end_symbol,
                          const std::vector<std::string>& alphabet, const std::vector<std::string>& separators, const char* out_dir,
                          std::string& err);
uint32_t lm_word_id(const HostLM& lm, const std::string& token);
double lm_model_score(const HostLM& lm, const uint32_t* ids, size_t n);
double lm_score_word_ids(const HostLM& lm, const uint32_t* ids, size_t n);
LmNext lm_model_next(const HostLM& lm, const uint32_t* ids, size_t n);
LmNext lm_next(const HostLM& lm, const uint32_t* ids, size_t n);
uint32_t lm_next_count(const HostLM& lm, const LmNext& nx, uint32_t word);
double lm_next_score(const HostLM& lm, const LmNext& nx, uint32_t word);
void lm_tokenize(const HostLM& lm, const uint8_t* text, size_t n, std::vector<std::string>& out);
void set_error(const std::string& msg);

// ---- the model's other two reference formats (lm_store.cpp; the device n-gram writer: lm_store.inc) ----
uint32_t mph_hash(uint32_t seed, const std::string& word);                  // mph.go:236-247
// mph.Build (pkg/mph/mph.go:40-145) over the words in id order: Get(word) = values[..] is its id
int mph_build(const std::vector<std::string>& words, std::vector<uint32_t>& values, std::vector<int32_t>& auxiliary, std::string& err);
int mph_section(const std::vector<std::string>& words, std::string& out, std::string& err);   // mph.Store's bytes
constexpr uint32_t kGmSliceBytes = 256u << 20;      // text of a level formatted, copied back and appended to its file at a time
uint32_t lm_gm_slice_budget(int64_t set);           // the budget in force; set >= 0: the test hook's value first (0 = kGmSliceBytes)
int lm_gm_check(const HostLM& lm, std::string& err);                        // SG_E_UNSUPPORTED: a model that cannot be spelled as lines
void lm_gm_parents(const LmLevel& lv, std::vector<uint32_t>& parent);       // parent[e] = the bucket that holds entry e
std::string lm_gm_path(const char* out_dir, size_t k);
struct GmFile {                                     // one <k>-gm being written; errors carry the path
  FILE* f = nullptr;
  std::string path;
  ~GmFile();
  int open(const std::string& p, std::string& err);
  int write(const void* data, size_t n, std::string& err);
  int close(std::string& err);
};
int lm_store_google_host(const HostLM& lm, const char* out_dir, double seconds[4], std::string& err);

// Values from outside the program (environment, sg_index_tune): a whole string, base 10, that fits an int32 — or nothing.
inline bool parse_int32(const char* s, int32_t* out) {
  char* end = nullptr;
  errno = 0;
  const long v = strtol(s, &end, 10);
  if (end == s || *end || errno || v < INT32_MIN || v > INT32_MAX) return false;
  *out = (int32_t)v;
  return true;
}
// A process-wide switch from the environment.  Unset or empty: def; not an integer of lo .. hi: a line on stderr and def (there is
// no call to fail).  The index's own knobs are the table of knobs.inc.
inline int32_t env_int(const char* name, int32_t lo, int32_t hi, int32_t def) {
  const char* e = getenv(name);
  if (!e || !*e) return def;
  int32_t v;
  if (parse_int32(e, &v) && v >= lo && v <= hi) return v;
  fprintf(stderr, "[suggest_hip] %s=%s: not an integer of %d .. %d, taking %d\n", name, e, lo, hi, def);
  return def;
}

}  // namespace sg
