// suggest_many_test.cpp — SuggestMany of the C++ mirror (include/suggest_hip.hpp): requests that differ in metric, similarity and
// topK answered by ONE mixed call give, request for request, what Service::Suggest-per-config batches (Service::SuggestBatch) give.
//
//   suggest_many_test --cpu <golden_dir>   host-side logic only: the checks SuggestMany makes before any device call
//   suggest_many_test <golden_dir>         + the searches on the cars dictionary: needs an MI355X
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

static void TestHost() {
  Service empty;
  const std::vector<SearchConfig> one{SearchConfig{"x", 1, metric::CosineMetric(), 0.5}};
  EXPECT(ErrorOf([&] { empty.SuggestMany("cars", one); }) == "given dictionary cars is not exists", "unknown dictionary");
  const std::vector<SearchConfig> bad_k{SearchConfig{"x", 0, metric::CosineMetric(), 0.5}};
  EXPECT(ErrorOf([&] { empty.SuggestMany("cars", bad_k); }) == "topK should be greater or equal to 1", "topK is checked per request");
  const std::vector<SearchConfig> bad_sim{SearchConfig{"x", 3, metric::CosineMetric(), 0.5}, SearchConfig{"y", 3, metric::DiceMetric(), 1.5}};
  EXPECT(ErrorOf([&] { empty.SuggestMany("cars", bad_sim); }) == "similarity shouble be in (0.0, 1.0]", "similarity is checked per request");
}

static void TestDevice(const std::string& golden) {
  const std::vector<IndexDescription> configs = ReadConfigs(golden + "/config.json");
  IndexDescription d = configs[0];
  d.driver = RAMDriver;
  Service svc;
  svc.AddIndexByDescription(d);
  const std::vector<std::string> queries{"nissan ma", "TOYOTA", "audi a4", "bmw x5", "Нива 2121", "mersedes benz", "ford focu", "honda civik", "opel astra", "volkswagen golf gti"};
  struct Key { metric::Metric m; double sim; int k; };
  const std::vector<Key> keys{{metric::JaccardMetric(), 0.5, 5}, {metric::CosineMetric(), 0.4, 10}, {metric::DiceMetric(), 0.3, 65},
                              {metric::ExactMetric(), 1.0, 1}, {metric::OverlapMetric(), 0.6, 3}, {metric::CosineMetric(), 0.4, 10}};
  std::vector<SearchConfig> reqs;
  for (size_t i = 0; i < 4 * queries.size(); i++) {          // every query under several keys, the keys interleaved
    const Key& k = keys[(i * 5 + i / 7) % keys.size()];
    reqs.push_back(NewSearchConfig(queries[i % queries.size()], k.k, k.m, k.sim));
  }
  std::vector<std::vector<ResultItem>> many;
  EXPECT(ErrorOf([&] { many = svc.SuggestMany("cars", reqs); }).empty(), "SuggestMany answers");
  EXPECT(many.size() == reqs.size(), "a row per request");
  size_t results = 0;
  for (size_t i = 0; i < reqs.size() && i < many.size(); i++) {
    std::vector<std::vector<ResultItem>> plain;
    const std::string err = ErrorOf([&] { plain = svc.SuggestBatch("cars", {reqs[i].query}, reqs[i].topK, reqs[i].metric, reqs[i].similarity); });
    EXPECT(err.empty() && plain.size() == 1, "the plain call answers");
    if (plain.size() != 1) continue;
    bool same = plain[0].size() == many[i].size();
    for (size_t j = 0; same && j < plain[0].size(); j++)
      same = std::memcmp(&plain[0][j].Score, &many[i][j].Score, 8) == 0 && plain[0][j].Value == many[i][j].Value;
    EXPECT(same, "request equals the plain call's row bit for bit");
    results += many[i].size();
  }
  EXPECT(results > 0, "the requests have results");
  EXPECT(svc.SuggestMany("cars", {}).empty(), "no requests, no rows");
}

int main(int argc, char** argv) {
  const bool cpu = argc > 1 && std::string(argv[1]) == "--cpu";
  if (argc < (cpu ? 3 : 2)) {
    std::fprintf(stderr, "usage: suggest_many_test [--cpu] <golden_dir>\n");
    return 2;
  }
  TestHost();
  if (!cpu) TestDevice(argv[argc - 1]);
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
