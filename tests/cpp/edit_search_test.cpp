// edit_search_test.cpp — the C++ mirror's complete search by edit distance (include/suggest_hip.hpp):
// dictionary::DeviceDictionary::EditSearch against literals and against a brute force written here — a two-row loop over bytes to
// every ASCII line of cars.dict, a sort by (distance, docID).
//
//   edit_search_test --cpu <golden_dir>   a host-resident handle only (no GPU)
//   edit_search_test <golden_dir>         + the same on a handle in HBM: needs an MI355X
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

static bool Same(const std::vector<EditCandidate>& row, std::initializer_list<std::pair<uint32_t, uint32_t>> want) {
  if (row.size() != want.size()) return false;
  size_t j = 0;
  for (auto& w : want) { if (row[j].Key != w.first || row[j].Distance != w.second) return false; j++; }
  return true;
}

static void TestLiterals(int device) {
  dictionary::DeviceDictionary d(std::vector<std::string>{"nissan", "toyota", "", "Toyota", "toyoat", "nisan"}, device);
  const std::vector<std::string> queries{"nisan", "toyota", "", std::string(65, 'a'), std::string(64, 'a')};
  std::vector<uint64_t> matches;
  auto rows = d.EditSearch(queries, 3, 2, false, true, &matches);
  EXPECT(rows.size() == 5 && Same(rows[0], {{5, 0}, {0, 1}}) && Same(rows[1], {{1, 0}, {3, 0}, {4, 2}}) && Same(rows[2], {{2, 0}}), "levenshtein, folded");
  EXPECT((matches == std::vector<uint64_t>{2, 3, 1, SG_COUNT_TOO_LONG, 0}) && rows[3].empty() && rows[4].empty(), "match counts; 65 runes flagged, 64 answered");
  rows = d.EditSearch(queries, 2, 1, true, false, &matches);
  EXPECT(Same(rows[1], {{1, 0}, {3, 1}}) && matches[1] == 3, "osa, unfolded: the transposition is one edit, k cuts the row, the count does not");
  EXPECT(ErrorOf([&] { d.EditSearch(queries, 3, 33); }) == "edit search: max_distance above 32", "max_distance is a true bound");
  EXPECT(ErrorOf([&] { d.EditSearch(queries, 0, 2); }) == "edit search: k should be in 1 .. 1024", "k is checked");
  EXPECT(d.EditSearch({}, 3, 2).empty(), "no queries");
}

static void TestAgainstTheLoop(const std::shared_ptr<dictionary::Dictionary>& host, int device) {
  std::vector<std::string> ascii;
  for (uint32_t i = 0; i < host->Size(); i++) if (Ascii(host->Get(i))) ascii.push_back(host->Get(i));
  dictionary::DeviceDictionary d(ascii, device);
  const std::vector<std::string> queries{"ACURA XL", "TOYOTA", "AUDI A44", "", "VOLKSWAGEN GOLF GTI", "X", "BMW X5", "FIRD FOCUS", "ACRUA TL", "acura el"};
  const int k = 10;
  for (const uint32_t md : {0u, 2u, 5u}) {
    std::vector<uint64_t> matches;
    const auto got = d.EditSearch(queries, k, md, false, false, &matches);
    bool same = got.size() == queries.size();
    size_t items = 0;
    for (size_t q = 0; same && q < queries.size(); q++) {
      std::vector<std::pair<uint32_t, uint32_t>> all;
      for (size_t j = 0; j < ascii.size(); j++) {
        const uint32_t dist = ByteLevenshtein(queries[q], ascii[j]);
        if (dist <= md) all.push_back({dist, (uint32_t)j});
      }
      std::sort(all.begin(), all.end());
      same = matches[q] == all.size() && got[q].size() == std::min<size_t>(all.size(), k);
      for (size_t j = 0; same && j < got[q].size(); j++) { same = got[q][j].Key == all[j].second && got[q][j].Distance == all[j].first; items++; }
    }
    EXPECT(same, "EditSearch equals the two-row loop to every ASCII line, sorted");
    EXPECT(md == 0 || items > 20, "the queries have matches");
  }
  EXPECT(ascii.size() > 1000, "most lines are ASCII");
}

int main(int argc, char** argv) {
  const bool cpu = argc > 1 && std::strcmp(argv[1], "--cpu") == 0;
  if (argc < (cpu ? 3 : 2)) {
    std::fprintf(stderr, "usage: edit_search_test [--cpu] <golden_dir>\n");
    return 2;
  }
  const std::string golden = argv[cpu ? 2 : 1];
  try {
    const std::vector<IndexDescription> configs = ReadConfigs(golden + "/config.json");
    const std::shared_ptr<dictionary::Dictionary> host = dictionary::OpenRAMDictionary(configs[0].GetSourcePath());
    TestLiterals(-1);
    TestAgainstTheLoop(host, -1);
    if (!cpu) {
      TestLiterals(0);
      TestAgainstTheLoop(host, 0);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL uncaught: %s\n", e.what());
    return 1;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
