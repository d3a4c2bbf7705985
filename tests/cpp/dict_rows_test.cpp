// dict_rows_test.cpp — the C++ mirror's DeviceDictionary (include/suggest_hip.hpp): Service::SuggestMany over a dictionary held
// in HBM gives, request for request, what the same Service gives over the host dictionary; Get / Size / Rows of the handle.
//
//   dict_rows_test --cpu <golden_dir>   a host-resident handle only (no GPU)
//   dict_rows_test <golden_dir>         + the cars dictionary on the device: needs an MI355X
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

static void TestHandle(const std::shared_ptr<dictionary::Dictionary>& host, int device) {
  dictionary::DeviceDictionary d(*host, device);
  EXPECT(d.Size() == host->Size() && d.Device() == device, "size and device");
  bool same = true;
  for (dictionary::Key k : {0u, 1u, 77u, (uint32_t)host->Size() - 1u}) same = same && d.Get(k) == host->Get(k);
  EXPECT(same, "Get");
  EXPECT(ErrorOf([&] { d.Get((dictionary::Key)host->Size()); }) == "key is not exists", "Get past the end");
  // two rows of three: the second flagged, the first with a count of two — and ids past the counts that must not be looked at
  const uint32_t ids[6] = {5, 9, 0xFFFFFFFFu, 1, 2, 3}, counts[2] = {2, SG_COUNT_TOO_LONG};
  std::vector<uint64_t> offs;
  const std::string text = d.Rows(ids, counts, nullptr, 2, 3, 6, offs);
  EXPECT(text == host->Get(5) + host->Get(9), "Rows: the text");
  EXPECT(offs.size() == 7 && offs[1] == host->Get(5).size() && offs[2] == text.size() && offs[6] == text.size(), "Rows: the offsets");
  const uint32_t outside[1] = {(uint32_t)host->Size()}, one[1] = {1};
  EXPECT(ErrorOf([&] { d.Rows(outside, one, nullptr, 1, 1, 1, offs); }) == "docID outside the dictionary", "an id outside is refused");
}

static void TestService(const std::string& golden) {
  const std::vector<IndexDescription> configs = ReadConfigs(golden + "/config.json");
  IndexDescription d = configs[0];
  d.driver = RAMDriver;
  const std::shared_ptr<dictionary::Dictionary> host = dictionary::OpenRAMDictionary(d.GetSourcePath());
  const auto on_device = std::make_shared<dictionary::DeviceDictionary>(*host, 0);
  Service svc;
  svc.AddIndex("host", host, NewRAMBuilder(host, d, 0));
  svc.AddIndex("device", on_device, NewRAMBuilder(host, d, 0));
  const std::vector<std::string> queries{"nissan ma", "TOYOTA", "audi a4", "bmw x5", "Нива 2121", "mersedes benz", "ford focu", "honda civik", "opel astra", "volkswagen golf gti", "zzzzqqq"};
  struct Key { metric::Metric m; double sim; int k; };
  const std::vector<Key> keys{{metric::JaccardMetric(), 0.5, 5}, {metric::CosineMetric(), 0.4, 10}, {metric::DiceMetric(), 0.3, 65}, {metric::ExactMetric(), 1.0, 1}};
  std::vector<SearchConfig> reqs;
  for (size_t i = 0; i < 4 * queries.size(); i++) {
    const Key& k = keys[(i * 3 + i / 5) % keys.size()];
    reqs.push_back(NewSearchConfig(queries[i % queries.size()], k.k, k.m, k.sim));
  }
  std::vector<std::vector<ResultItem>> a, b;
  EXPECT(ErrorOf([&] { a = svc.SuggestMany("host", reqs); }).empty(), "the host dictionary answers");
  EXPECT(ErrorOf([&] { b = svc.SuggestMany("device", reqs); }).empty(), "the device dictionary answers");
  EXPECT(a.size() == reqs.size() && b.size() == reqs.size(), "a row per request");
  size_t items = 0;
  bool same = a.size() == b.size();
  for (size_t i = 0; same && i < a.size(); i++) {
    same = a[i].size() == b[i].size();
    for (size_t j = 0; same && j < a[i].size(); j++) {
      same = a[i][j].Value == b[i][j].Value && std::memcmp(&a[i][j].Score, &b[i][j].Score, 8) == 0;
      items++;
    }
  }
  EXPECT(same, "equal values and score bits, request for request");
  EXPECT(items > 100, "the requests have results");
  // Suggest and Autocomplete go through Dictionary::Get: a DeviceDictionary is a Dictionary
  const SearchConfig one = NewSearchConfig("nissan ma", 5, metric::CosineMetric(), 0.4);
  const auto sa = svc.Suggest("host", one), sb = svc.Suggest("device", one);
  bool same_one = sa.size() == sb.size() && !sa.empty();
  for (size_t j = 0; same_one && j < sa.size(); j++) same_one = sa[j].Value == sb[j].Value;
  EXPECT(same_one, "Suggest over the device dictionary");
  TestHandle(host, 0);
}

int main(int argc, char** argv) {
  const bool cpu = argc > 1 && std::strcmp(argv[1], "--cpu") == 0;
  if (argc < (cpu ? 3 : 2)) {
    std::fprintf(stderr, "usage: dict_rows_test [--cpu] <golden_dir>\n");
    return 2;
  }
  const std::string golden = argv[cpu ? 2 : 1];
  try {
    const std::vector<IndexDescription> configs = ReadConfigs(golden + "/config.json");
    TestHandle(dictionary::OpenRAMDictionary(configs[0].GetSourcePath()), -1);
    if (!cpu) TestService(golden);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL uncaught: %s\n", e.what());
    return 1;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
