// index_store.cpp — saves an index in the reference's on-disk format, the counterpart of ref_index_reader.cpp:
//   <name>.dl  the posting lists back to back, codec by RAW length (index.NewEncoder, pkg/index/codec.go:17-51):
//              <= 65 VB deltas (compression/varint.go:36-55), <= 256 skip blocks of 64 (compression/skipping.go:67-113),
//              else roaring v0.5.5 WriteTo after RunOptimize over the de-duplicated docIDs (compression/bitmap.go:18-29)
//   <name>.hd  the gob stream of header{Version "v5.1", Indices, Terms []termDescription} (Writer.Commit,
//              pkg/index/indexer_writer.go:50-63,88-167), terms in the order segment ascending, then sg_index_lists' order
//              (the reference walks a Go map: its order is random)
// This file holds the list table, the plain host encoder (the restatement the kernels of index_store.inc are read against),
// the position scan and the two file writers.  Only the byte formats are restated; no reference code is used.

#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>

#include "sg_internal.h"

namespace sg {

// The non-empty lists in header order with their slices of `dups`.  dups is sorted by (term, segment, doc), so a list's
// marker entry (doc == 0xFFFFFFFF: a reference-built roaring list that had already dropped its repeats) ends its slice.
int store_lists(const HostIndex& ix, std::vector<StoreList>& out, std::string& err) {
  const size_t S = ix.n_segments, nT = ix.term_key.size();
  out.clear();
  out.reserve((size_t)ix.n_lists);
  std::vector<uint32_t> dup_at(nT + 1, 0);                       // first entry of dups per term
  {
    size_t d = 0;
    for (size_t t = 0; t <= nT; t++) {
      while (d < ix.dups.size() && ix.dups[d].term < t) d++;
      dup_at[t] = (uint32_t)d;
    }
  }
  for (size_t b = 0; b < S; b++)
    for (size_t t = 0; t < nT; t++) {
      const uint32_t len = ix.list_len[t * S + b];
      if (!len) continue;
      StoreList l{};
      l.src = (uint64_t)ix.seg_off[t * (S + 1) + b] * 4;
      l.term = (uint32_t)t; l.segment = (uint32_t)b; l.len = len;
      uint64_t raw = len;
      uint32_t d = dup_at[t];
      while (d < dup_at[t + 1] && ix.dups[d].segment < b) d++;
      l.dup_begin = d;
      for (; d < dup_at[t + 1] && ix.dups[d].segment == b; d++) {
        raw += ix.dups[d].mult - 1;                               // mult = how often the document holds the term (sg_index_list)
        if (ix.dups[d].doc != 0xFFFFFFFFu) l.dup_n++;
      }
      if (raw > 0xFFFFFFFFull) { err = "a posting list's raw length exceeds 32 bits"; return SG_E_UNSUPPORTED; }
      l.raw = (uint32_t)raw;
      out.push_back(l);
    }
  return SG_OK;
}

namespace {

inline void put_varint(std::vector<uint8_t>& o, uint32_t v) {
  while (v >= 0x80u) { o.push_back((uint8_t)(v | 0x80u)); v >>= 7; }
  o.push_back((uint8_t)v);
}
inline void put_u16(std::vector<uint8_t>& o, uint32_t v) { o.push_back((uint8_t)v); o.push_back((uint8_t)(v >> 8)); }
inline void put_u32(std::vector<uint8_t>& o, uint32_t v) { put_u16(o, v & 0xFFFFu); put_u16(o, v >> 16); }

// roaring portable serialisation of the ascending, distinct v[0 .. n).  A container of cardinality c in r runs is a run
// container when 2 + 4r <= min(8192, 2c) (ties go to the run), else an array up to 4096 values, else a bitmap.
void encode_roaring(const uint32_t* v, size_t n, std::vector<uint8_t>& o) {
  struct Cont { uint32_t key, card, runs, size; size_t beg; bool is_run; };
  std::vector<Cont> cs;
  bool any_run = false;
  for (size_t i = 0; i < n;) {
    Cont c{v[i] >> 16, 0, 0, 0, i, false};
    size_t j = i;
    for (; j < n && (v[j] >> 16) == c.key; j++) c.runs += j == i || v[j] != v[j - 1] + 1;
    c.card = (uint32_t)(j - i);
    c.is_run = 2 + 4 * (uint64_t)c.runs <= std::min<uint64_t>(8192, 2 * (uint64_t)c.card);
    c.size = c.is_run ? 2 + 4 * c.runs : c.card <= 4096 ? 2 * c.card : 8192;
    any_run |= c.is_run;
    cs.push_back(c);
    i = j;
  }
  const uint32_t nc = (uint32_t)cs.size();
  const bool offsets = !any_run || nc >= 4;
  uint32_t head;
  if (any_run) {
    put_u32(o, 12347u | ((nc - 1) << 16));
    for (uint32_t b = 0; b < (nc + 7) / 8; b++) {
      uint8_t f = 0;
      for (uint32_t k = 0; k < 8 && 8 * b + k < nc; k++) f |= (uint8_t)(cs[8 * b + k].is_run << k);
      o.push_back(f);
    }
    head = 4 + (nc + 7) / 8;
  } else {
    put_u32(o, 12346u); put_u32(o, nc);
    head = 8;
  }
  for (const Cont& c : cs) { put_u16(o, c.key); put_u16(o, c.card - 1); }
  head += 4 * nc + (offsets ? 4 * nc : 0);
  if (offsets) { uint32_t off = head; for (const Cont& c : cs) { put_u32(o, off); off += c.size; } }
  for (const Cont& c : cs) {
    const uint32_t* p = v + c.beg;
    if (c.is_run) {
      put_u16(o, c.runs);
      for (uint32_t i = 0; i < c.card;) {
        uint32_t j = i + 1;
        while (j < c.card && p[j] == p[j - 1] + 1) j++;
        put_u16(o, p[i] & 0xFFFFu); put_u16(o, j - i - 1);
        i = j;
      }
    } else if (c.card <= 4096) {
      for (uint32_t i = 0; i < c.card; i++) put_u16(o, p[i] & 0xFFFFu);
    } else {
      const size_t at = o.size();
      o.resize(at + 8192, 0);
      for (uint32_t i = 0; i < c.card; i++) { const uint32_t x = p[i] & 0xFFFFu; o[at + (x >> 3)] |= (uint8_t)(1u << (x & 7)); }
    }
  }
}

struct Gob {   // encoding/gob's wire forms of the values the header needs
  std::string b;
  void u(uint64_t v) {
    if (v < 128) { b.push_back((char)v); return; }
    int n = 0;
    for (uint64_t x = v; x; x >>= 8) n++;
    b.push_back((char)(256 - n));
    for (int k = n - 1; k >= 0; k--) b.push_back((char)(v >> (8 * k)));
  }
  void i(int64_t v) { u(v < 0 ? ((uint64_t)~v << 1) | 1 : (uint64_t)v << 1); }
  void s(const std::string& x) { u(x.size()); b += x; }
  void message(const Gob& body) { u(body.b.size()); b += body.b; }
};

constexpr int kGobUint = 3, kGobString = 6;                         // encoding/gob's built-in type ids
constexpr int kIdHeader = 65, kIdTerm = 66, kIdTerms = 67;          // the ids a fresh encoder hands out, in the order it meets the types

struct GobField { const char* name; int type; };

// wireType{StructT: &structType{CommonType{Name, Id}, Field []fieldType{Name, Id}}}
void gob_define_struct(Gob& out, int id, const char* name, std::initializer_list<GobField> fields) {
  Gob m;
  m.i(-id);
  m.u(3);                                                            // wireType.StructT is field 2
  m.u(1); m.u(1); m.s(name); m.u(1); m.i(id); m.u(0);                // CommonType
  m.u(1); m.u(fields.size());
  for (const GobField& f : fields) { m.u(1); m.s(f.name); m.u(1); m.i(f.type); m.u(0); }
  m.u(0); m.u(0);
  out.message(m);
}
// wireType{SliceT: &sliceType{CommonType{Name, Id}, Elem}}
void gob_define_slice(Gob& out, int id, const char* name, int elem) {
  Gob m;
  m.i(-id);
  m.u(2);                                                            // wireType.SliceT is field 1
  m.u(1); m.u(1); m.s(name); m.u(1); m.i(id); m.u(0);
  m.u(1); m.i(elem);
  m.u(0); m.u(0);
  out.message(m);
}

std::string term_string(const HostIndex& ix, uint64_t key) {        // the reference's term string of a packed key (sg_term_string)
  std::string s;
  for (int i = 0; i < 8; i++) {
    const uint32_t id = (key >> (8 * i)) & 0xFF;
    if (!id || id >= ix.sym.sym_rune.size()) break;
    const uint32_t r = ix.sym.sym_rune[id];
    if (r < 0x80) s.push_back((char)r);
    else if (r < 0x800) { s.push_back((char)(0xC0 | (r >> 6))); s.push_back((char)(0x80 | (r & 0x3F))); }
    else if (r < 0x10000) { s.push_back((char)(0xE0 | (r >> 12))); s.push_back((char)(0x80 | ((r >> 6) & 0x3F))); s.push_back((char)(0x80 | (r & 0x3F))); }
    else { s.push_back((char)(0xF0 | (r >> 18))); s.push_back((char)(0x80 | ((r >> 12) & 0x3F))); s.push_back((char)(0x80 | ((r >> 6) & 0x3F))); s.push_back((char)(0x80 | (r & 0x3F))); }
  }
  return s;
}

bool write_file(const char* path, const char* a, size_t na, const char* b, size_t nb, std::string& err) {
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  if (f) { if (na) f.write(a, (std::streamsize)na); if (nb) f.write(b, (std::streamsize)nb); f.close(); }
  if (!f) { err = std::string("failed to write ") + path; return false; }
  return true;
}

}  // namespace

void store_encode_host(const HostIndex& ix, const std::vector<StoreList>& lists, std::vector<uint32_t>& size, std::vector<uint8_t>& dl) {
  size.assign(lists.size(), 0);
  dl.clear();
  std::vector<uint32_t> raw;
  for (size_t li = 0; li < lists.size(); li++) {
    const StoreList& l = lists[li];
    const uint32_t* p = ix.postings.data() + l.src;
    const size_t at = dl.size();
    if (l.raw > 256) encode_roaring(p, l.len, dl);
    else {
      raw.clear();                                                   // the raw list: a repeated document as often as it holds the term
      uint32_t d = l.dup_begin;
      for (uint32_t i = 0; i < l.len; i++) {
        uint32_t m = 1;
        if (d < l.dup_begin + l.dup_n && ix.dups[d].doc == p[i]) m = std::max(ix.dups[d++].mult, 1u);
        raw.insert(raw.end(), m, p[i]);
      }
      if (l.raw <= 65) {
        uint32_t prev = 0;
        for (uint32_t x : raw) { put_varint(dl, x - prev); prev = x; }
      } else {
        uint32_t block_first = 0;
        for (size_t b0 = 0; b0 < raw.size(); b0 += 64) {
          const size_t b1 = std::min(raw.size(), b0 + 64), head = dl.size();
          put_u16(dl, 0);
          uint32_t prev = block_first;                               // a block's first value: a delta to the previous block's first
          for (size_t i = b0; i < b1; i++) { put_varint(dl, raw[i] - prev); prev = raw[i]; }
          block_first = raw[b0];
          const uint32_t bytes = (uint32_t)(dl.size() - head) | (b1 == raw.size() ? 0x8000u : 0u);
          dl[head] = (uint8_t)bytes; dl[head + 1] = (uint8_t)(bytes >> 8);
        }
      }
    }
    size[li] = (uint32_t)(dl.size() - at);
  }
}

int store_positions(const std::vector<uint32_t>& size, std::vector<uint32_t>& pos, uint64_t* total, std::string& err) {
  pos.resize(size.size());
  uint64_t at = 0;
  for (size_t i = 0; i < size.size(); i++) { pos[i] = (uint32_t)at; at += size[i]; }
  *total = at;
  if (at >= (1ull << 32)) { err = "the document list file would reach 4 GiB: PostingListPosition is a uint32"; return SG_E_UNSUPPORTED; }
  return SG_OK;
}

int store_write_files(const HostIndex& ix, const std::vector<StoreList>& lists, const std::vector<uint32_t>& size,
                      const std::vector<uint32_t>& pos, const uint8_t* dl, uint64_t dl_bytes, const char* hd_path, const char* dl_path,
                      double* header_seconds, std::string& err) {
  const auto t0 = std::chrono::steady_clock::now();
  Gob hd;
  gob_define_struct(hd, kIdHeader, "header", {{"Version", kGobString}, {"Indices", kGobUint}, {"Terms", kIdTerms}});
  gob_define_slice(hd, kIdTerms, "[]index.termDescription", kIdTerm);
  gob_define_struct(hd, kIdTerm, "termDescription", {{"Term", kGobString}, {"Indice", kGobUint}, {"PostingListBytesSize", kGobUint},
                                                     {"PostingListPosition", kGobUint}, {"PostingListLen", kGobUint}});
  Gob v;                                                             // the value: struct fields as deltas, zero values left out
  v.b.reserve(lists.size() * 24 + 64);
  v.i(kIdHeader);
  int field = -1;
  v.u(0 - field); v.s("v5.1"); field = 0;
  if (ix.n_segments) { v.u(1 - field); v.u(ix.n_segments); field = 1; }
  if (!lists.empty()) {
    v.u(2 - field); v.u(lists.size());
    for (size_t i = 0; i < lists.size(); i++) {
      const std::string term = term_string(ix, ix.term_key[lists[i].term]);
      const uint64_t vals[5] = {0, lists[i].segment, size[i], pos[i], lists[i].raw};
      int f = -1;
      if (!term.empty()) { v.u(1); v.s(term); f = 0; }
      for (int k = 1; k < 5; k++)
        if (vals[k]) { v.u(k - f); v.u(vals[k]); f = k; }
      v.u(0);
    }
  }
  v.u(0);
  Gob len;
  len.u(v.b.size());
  hd.b += len.b;
  const auto t1 = std::chrono::steady_clock::now();
  if (!write_file(dl_path, (const char*)dl, (size_t)dl_bytes, nullptr, 0, err)) return SG_E_INVALID;
  const auto t2 = std::chrono::steady_clock::now();
  if (!write_file(hd_path, hd.b.data(), hd.b.size(), v.b.data(), v.b.size(), err)) return SG_E_INVALID;
  if (header_seconds) *header_seconds = std::chrono::duration<double>(t1 - t0).count() + std::chrono::duration<double>(std::chrono::steady_clock::now() - t2).count();
  return SG_OK;
}

}  // namespace sg
