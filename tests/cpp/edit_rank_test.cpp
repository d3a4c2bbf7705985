// edit_rank_test.cpp — the C++ mirror's edit-distance ranking (include/suggest_hip.hpp):
// dictionary::DeviceDictionary::EditDistances against literals and a two-row loop over bytes written here, NGramIndex::SuggestEdit
// against the composition of SuggestBatch(k = candidates), the host-resident handle's distances and a stable sort.
//
//   edit_rank_test --cpu <golden_dir>   a host-resident handle only (no GPU)
//   edit_rank_test <golden_dir>         + the handle and the cars index on the device: needs an MI355X
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../include/suggest_hip.hpp"

using namespace suggest;

static int g_failed = 0, g_checks = 0;
#define EXPECT(cond, what)                                               \
  do {                                                                   \
    g_checks++;                                                          \
    if (!(cond)) {                                                       \
      g_failed++;                                                        \
      std::fprintf(stderr, "FAIL %s:%d  %s\n", __FILE__, __LINE__, what); \
    }                                                                    \
  } while (0)

template <class F>
static std::string ErrorOf(F f) {
  try {
    f();
  } catch (const Error& e) {
    return e.what();
  }
  return "";
}

static const uint32_t kNone = 0xFFFFFFFFu;

static bool Ascii(const std::string& s) {
  for (unsigned char c : s) if (c >= 0x80) return false;
  return true;
}
// Levenshtein over bytes: equal to the distance over runes for ASCII strings, unfolded
static uint32_t ByteLevenshtein(const std::string& a, const std::string& b) {
  std::vector<uint32_t> prev(a.size() + 1), cur(a.size() + 1);
  for (size_t i = 0; i <= a.size(); i++) prev[i] = (uint32_t)i;
  for (size_t j = 1; j <= b.size(); j++) {
    cur[0] = (uint32_t)j;
    for (size_t i = 1; i <= a.size(); i++) cur[i] = std::min(std::min(prev[i] + 1, cur[i - 1] + 1), prev[i - 1] + (a[i - 1] != b[j - 1] ? 1u : 0u));
    prev.swap(cur);
  }
  return prev[a.size()];
}

static void TestLiterals(int device) {
  dictionary::DeviceDictionary d(std::vector<std::string>{"nissan", "toyota", "", "TOYOTA corolla"}, device);
  const uint32_t ids[8] = {0, 1, 2, 3, 1, 7, 3, 0}, counts[2] = {3, 3};
  const std::vector<std::string> queries{"nisan", "toyoat"};
  // (the id 7 is outside the dictionary: refused, after the rest was computed)
  EXPECT(ErrorOf([&] { d.EditDistances(queries, ids, counts, nullptr, 4, 8, true); }) == "docID outside the dictionary", "an id outside is refused");
  const uint32_t ids2[8] = {0, 1, 2, 3, 1, 2, 3, 0};
  EXPECT((d.EditDistances(queries, ids2, counts, nullptr, 4, 8, true) == std::vector<uint32_t>{1, 6, 5, kNone, 1, 6, 9, kNone}), "osa, folded");
  EXPECT((d.EditDistances(queries, ids2, counts, nullptr, 4, 8, false) == std::vector<uint32_t>{1, 6, 5, kNone, 2, 6, 9, kNone}), "levenshtein, folded");
  const uint32_t flagged[2] = {SG_COUNT_TOO_LONG, 1};
  EXPECT((d.EditDistances(queries, ids2, flagged, nullptr, 4, 8, false, false) == std::vector<uint32_t>{kNone, kNone, kNone, kNone, 2, kNone, kNone, kNone}),
         "a flagged row, a count of one");
  const uint64_t ragged[3] = {0, 1, 4};
  const uint32_t rc[2] = {1, 9};
  EXPECT((d.EditDistances(queries, ids2, rc, ragged, 0, 8, true) == std::vector<uint32_t>{1, 1, 6, 9, kNone, kNone, kNone, kNone}), "ragged rows");
  EXPECT(ErrorOf([&] { d.EditDistances(queries, ids2, counts, nullptr, 5, 8); }) == "dictionary rows: slots is below n_rows * row", "the geometry is checked");
}

static void TestAgainstTheLoop(const std::shared_ptr<dictionary::Dictionary>& host, int device) {
  dictionary::DeviceDictionary d(*host, device);
  std::vector<uint32_t> ascii;
  for (uint32_t i = 0; i < host->Size() && ascii.size() < 400; i += 7) if (Ascii(host->Get(i))) ascii.push_back(i);
  const std::vector<std::string> queries{"nissan ma", "TOYOTA", "audi a4", "", "volkswagen golf gti", "x"};
  std::vector<uint32_t> ids, counts(queries.size(), (uint32_t)ascii.size());
  for (size_t q = 0; q < queries.size(); q++) ids.insert(ids.end(), ascii.begin(), ascii.end());
  const std::vector<uint32_t> got = d.EditDistances(queries, ids.data(), counts.data(), nullptr, (uint32_t)ascii.size(), ids.size(), false, false);
  bool same = got.size() == ids.size();
  for (size_t q = 0; same && q < queries.size(); q++)
    for (size_t j = 0; same && j < ascii.size(); j++) same = got[q * ascii.size() + j] == ByteLevenshtein(queries[q], host->Get(ascii[j]));
  EXPECT(ascii.size() > 100 && same, "EditDistances equals the two-row loop on the ASCII lines");
}

static void TestSuggestEdit(const std::string& golden) {
  const std::vector<IndexDescription> configs = ReadConfigs(golden + "/config.json");
  IndexDescription desc = configs[0];
  desc.driver = RAMDriver;
  const std::shared_ptr<dictionary::Dictionary> host = dictionary::OpenRAMDictionary(desc.GetSourcePath());
  const dictionary::DeviceDictionary on_device(*host, 0), on_host(*host, -1);
  const std::shared_ptr<NGramIndex> ix = NewRAMBuilder(host, desc, 0)->Build();
  const std::vector<std::string> queries{"nissan ma", "TOYTOA", "audi a4", "bmw x5", "Нива 2121", "mersedes benz", "ford focu", "honda civik", "opel astar", "zzzzqqq", ""};
  for (const bool osa : {false, true}) {
    EditDistance rr;
    rr.candidates = 64; rr.transpositions = osa; rr.max_distance = osa ? 0xFFFFFFFFu : 6u;
    const int k = 10;
    std::vector<std::vector<EditCandidate>> got;
    EXPECT(ErrorOf([&] { got = ix->SuggestEdit(on_device, queries, 0.3, metric::JaccardMetric(), k, rr); }).empty(), "SuggestEdit answers");
    const auto cand = ix->SuggestBatch(queries, 0.3, metric::JaccardMetric(), rr.candidates);
    bool same = got.size() == queries.size();
    size_t items = 0;
    for (size_t i = 0; same && i < queries.size(); i++) {
      std::vector<uint32_t> ids, counts{(uint32_t)cand[i].size()};
      for (auto& c : cand[i]) ids.push_back(c.Key);
      ids.resize(rr.candidates, 0);
      const std::vector<uint32_t> dist = on_host.EditDistances({queries[i]}, ids.data(), counts.data(), nullptr, (uint32_t)rr.candidates, ids.size(), osa);
      std::vector<size_t> order(cand[i].size());
      for (size_t p = 0; p < order.size(); p++) order[p] = p;
      std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return dist[x] < dist[y]; });
      std::vector<size_t> keep;
      for (size_t p : order) if (dist[p] <= rr.max_distance && keep.size() < (size_t)k) keep.push_back(p);
      same = got[i].size() == keep.size();
      for (size_t j = 0; same && j < keep.size(); j++) {
        same = got[i][j].Key == cand[i][keep[j]].Key && got[i][j].Distance == dist[keep[j]] && std::memcmp(&got[i][j].Score, &cand[i][keep[j]].Score, 8) == 0;
        items++;
      }
    }
    EXPECT(same, "SuggestEdit = SuggestBatch(candidates) + host distances + a stable sort, row for row");
    EXPECT(items > 30, "the queries have results");
  }
  EXPECT(!ErrorOf([&] { ix->SuggestEdit(on_device, queries, 0.3, metric::JaccardMetric(), 65); }).empty(), "topK above the candidates is refused");
  EXPECT(!ErrorOf([&] { ix->SuggestEdit(on_host, queries, 0.3, metric::JaccardMetric(), 5); }).empty(), "a host-resident dictionary is refused");
  TestLiterals(0);
  TestAgainstTheLoop(host, 0);
}

int main(int argc, char** argv) {
  const bool cpu = argc > 1 && std::strcmp(argv[1], "--cpu") == 0;
  if (argc < (cpu ? 3 : 2)) {
    std::fprintf(stderr, "usage: edit_rank_test [--cpu] <golden_dir>\n");
    return 2;
  }
  const std::string golden = argv[cpu ? 2 : 1];
  try {
    const std::vector<IndexDescription> configs = ReadConfigs(golden + "/config.json");
    TestLiterals(-1);
    TestAgainstTheLoop(dictionary::OpenRAMDictionary(configs[0].GetSourcePath()), -1);
    if (!cpu) TestSuggestEdit(golden);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL uncaught: %s\n", e.what());
    return 1;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
