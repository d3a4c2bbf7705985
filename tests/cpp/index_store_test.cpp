// index_store_test.cpp — suggest::Index (pkg/suggest/indexer.go:14-45 and the `indexer` command) of the C++ mirror:
// indexes tests/golden/cars.dict into <out_dir>/cars.hd, .dl and .cdb, and opens the result again.
//
//   index_store_test --cpu <golden_dir> <out_dir>   built and encoded on the host; the files load (sg_index_load_reference) into
//                                                   the CSR the dictionary builds, the .cdb equals the reference's own
//   index_store_test <golden_dir> <out_dir>         built and encoded on GPU 0; NewFSBuilder opens the result and answers the
//                                                   suggest_auto / autocomplete queries of reference_tests.json (and a few
//                                                   more) as the index built in memory does; the reference's small collection
//                                                   goes the same way and answers with the ids its Go tests expect (the
//                                                   expected_ids of reference_tests.json): needs an MI355X
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

static bool SameRows(const std::vector<Candidate>& a, const std::vector<Candidate>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].Key != b[i].Key || std::memcmp(&a[i].Score, &b[i].Score, sizeof(double)) != 0) return false;
  return true;
}

int main(int argc, char** argv) {
  const bool cpu = argc > 1 && std::string(argv[1]) == "--cpu";
  if (argc != (cpu ? 4 : 3)) {
    std::fprintf(stderr, "usage: index_store_test [--cpu] <golden_dir> <out_dir>\n");
    return 2;
  }
  const std::string golden = argv[cpu ? 2 : 1], out = argv[cpu ? 3 : 2];
  try {
    IndexDescription d = ReadConfigs(golden + "/config.json")[0];          // the reference's own description of cars
    auto dict = dictionary::OpenRAMDictionary(d.GetSourcePath());
    d.basePath = out;
    d.OutputPath = ".";
    Index(d, dict, cpu ? -1 : 0);

    // the dictionary: byte for byte the reference's cdb, and it opens
    EXPECT(dictionary::ReadFile(d.GetDictionaryFile(), "cdb") == dictionary::ReadFile(golden + "/db/cars.cdb", "cdb"), "cars.cdb equals the reference's");
    auto cdb = dictionary::OpenCDBDictionary(d.GetDictionaryFile());
    bool same = cdb->Size() == dict->Size();
    for (uint32_t i = 0; same && i < dict->Size(); i++) same = cdb->Get(i) == dict->Get(i);
    EXPECT(same, "cdb == lines");
    EXPECT(dictionary::ReadFile(d.GetDocumentListFile(), "dl").size() == dictionary::ReadFile(golden + "/db/cars.dl", "dl").size(), "cars.dl has the reference's size");

    if (cpu) {                                                              // the files load into the CSR the dictionary builds
      detail::DescC dc(d);
      sg_index *loaded = nullptr, *built = nullptr;
      NGramIndex::Check(sg_index_load_reference(d.GetHeaderFile().c_str(), d.GetDocumentListFile().c_str(), &dc.d, &loaded));
      NGramIndex a(loaded);
      std::string blob;
      std::vector<uint64_t> offs(1, 0);
      dict->Iterate([&](dictionary::Key, const dictionary::Value& w) { blob += w; offs.push_back(blob.size()); });
      NGramIndex::Check(sg_index_build((const uint8_t*)blob.data(), offs.data(), (uint32_t)(offs.size() - 1), &dc.d, &built));
      NGramIndex b(built);
      sg_stats sa{}, sb{};
      NGramIndex::Check(sg_index_stats(loaded, &sa));
      NGramIndex::Check(sg_index_stats(built, &sb));
      EXPECT(sa.n_docs == sb.n_docs && sa.n_segments == sb.n_segments && sa.n_terms == sb.n_terms && sa.n_lists == sb.n_lists &&
                 sa.n_postings == sb.n_postings && sa.n_postings_raw == sb.n_postings_raw, "statistics of the reloaded index");
      const uint64_t n = sg_index_lists(built, nullptr, nullptr, 0);
      std::vector<uint32_t> segs(n), x(1 << 16), y(1 << 16);
      std::vector<uint64_t> keys(n);
      sg_index_lists(built, segs.data(), keys.data(), n);
      bool lists_same = n == sg_index_lists(loaded, nullptr, nullptr, 0);
      for (uint64_t i = 0; lists_same && i < n; i++) {
        uint64_t ra = 0, rb = 0;
        const int64_t la = sg_index_list(loaded, segs[i], keys[i], x.data(), x.size(), &ra), lb = sg_index_list(built, segs[i], keys[i], y.data(), y.size(), &rb);
        lists_same = la == lb && ra == rb && la >= 0 && (size_t)la <= x.size() && std::memcmp(x.data(), y.data(), (size_t)la * 4) == 0;
      }
      EXPECT(lists_same, "every list of the reloaded index");
    } else {
      auto fs = NewFSBuilder(d)->Build();
      auto ram = NewRAMBuilder(dict, d)->Build();
      const Json ref = Json::Parse(dictionary::ReadFile(golden + "/reference_tests.json", "golden"));
      std::vector<std::string> queries = {ref.at("suggest_auto").at("query").str, ref.at("autocomplete").at("query").str,
                                          "Nissan Maxima", "toyota corola", "mersedes", "bmw x5", "Шкода"};
      for (const std::string& q : queries) {
        for (double alpha : {0.3, 0.5}) {
          EXPECT(SameRows(fs->Suggest(q, alpha, metric::JaccardMetric(), 10), ram->Suggest(q, alpha, metric::JaccardMetric(), 10)), ("Suggest " + q).c_str());
          EXPECT(SameRows(fs->Suggest(q, alpha, metric::CosineMetric(), 7), ram->Suggest(q, alpha, metric::CosineMetric(), 7)), ("Suggest cosine " + q).c_str());
        }
        EXPECT(SameRows(fs->Autocomplete(q, 20), ram->Autocomplete(q, 20)), ("Autocomplete " + q).c_str());
      }
      EXPECT(!ram->Suggest("Nissan Maxima", 0.5, metric::JaccardMetric(), 10).empty(), "the queries find something");

      // the reference's own expectations (ngram_index_test.go:15-67, as recorded in reference_tests.json): its small collection
      // indexed to files, opened with NewFSBuilder, answers with the ids the Go tests expect
      std::vector<std::string> collection;
      for (const Json& x : ref.at("small_collection").arr) collection.push_back(x.str);
      auto small = dictionary::NewInMemoryDictionary(collection);
      for (const char* which : {"suggest_auto", "autocomplete"}) {
        const Json& t = ref.at(which);
        IndexDescription s;
        s.Name = std::string("small_") + which;
        s.NGramSize = (int)t.at("description").at("nGramSize").num;
        s.Pad = t.at("description").at("pad").str;
        s.Wrap[0] = t.at("description").at("wrap").at(0).str;
        s.Wrap[1] = t.at("description").at("wrap").at(1).str;
        for (const Json& a : t.at("description").at("alphabet").arr) s.Alphabet.push_back(a.str);
        s.basePath = out;
        s.OutputPath = ".";
        Index(s, small, 0);
        auto opened = NewFSBuilder(s)->Build();
        const bool fuzzy = std::string(which) == "suggest_auto";
        const std::vector<Candidate> got = fuzzy ? opened->Suggest(t.at("query").str, t.at("similarity").num, metric::JaccardMetric(), (int)t.at("topK").num)
                                                 : opened->Autocomplete(t.at("query").str, (int)t.at("limit").num);
        bool ok = got.size() == t.at("expected_ids").size();
        for (size_t i = 0; ok && i < got.size(); i++) ok = got[i].Key == (uint32_t)t.at("expected_ids").at(i).num;
        EXPECT(ok, (std::string(which) + ": the ids the reference's test expects").c_str());
        EXPECT(!fuzzy || t.at("metric").str == "jaccard", "suggest_auto is a Jaccard query");
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL exception: %s\n", e.what());
    g_failed++;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
