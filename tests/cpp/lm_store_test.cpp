// lm_store_test.cpp — mph_build and the host n-gram writer (suggest_amd/csrc/lm_store.cpp) as a stand-alone program: compiled
// with the host sources themselves under AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_lm_ngrams_cpu.py.
//   lm_store_test <golden lm directory> <scratch directory>
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../suggest_amd/csrc/sg_internal.h"

namespace sg { void set_error(const std::string&) {} }      // (the library's lives with the C ABI, which is not linked here)

static int failed = 0, passed = 0;
#define CHECK(cond) do { if (cond) passed++; else { failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static std::vector<std::string> sorted_lines(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<std::string> out;
  for (std::string l; std::getline(f, l);) out.push_back(l);
  std::sort(out.begin(), out.end());
  return out;
}
static uint32_t mph_get(const std::vector<uint32_t>& values, const std::vector<int32_t>& aux, const std::string& w) {   // mph.go:148-156
  const int32_t d = aux[sg::mph_hash(0, w) % aux.size()];
  if (d < 0) return values[(size_t)(-d - 1)];
  return values[sg::mph_hash((uint32_t)d, w) % values.size()];
}

int main(int argc, char** argv) {
  if (argc < 3) { printf("usage: lm_store_test <golden lm directory> <scratch directory>\n"); return 2; }
  const std::string golden = argv[1], scratch = argv[2];
  const std::vector<std::string> alphabet = {"english", "russian", "numbers", "-."};
  std::string err;

  // the fixture: the model of 1/2/3-gm numbered like the production build; test.lm = its model section + the MPH
  sg::HostLM lm;
  CHECK(sg::lm_load_google(golden.c_str(), 3, "<S>", "</S>", alphabet, 1, lm, err) == SG_OK);
  CHECK(lm.words.size() == 12);
  std::string section;
  CHECK(sg::mph_section(lm.words, section, err) == SG_OK);
  const std::string file = slurp(golden + "/test.lm");
  CHECK(file.size() == 658 && section.size() == 104);
  CHECK(file.size() >= section.size() && file.compare(file.size() - section.size(), section.size(), section) == 0);
  CHECK(sg::lm_store_binary(lm, (scratch + "/t.lm").c_str(), (scratch + "/t.cdb").c_str(), SG_LM_STORE_MPH, err) == SG_OK);
  CHECK(slurp(scratch + "/t.lm") == file);
  CHECK(slurp(scratch + "/t.cdb") == slurp(golden + "/test.cdb"));

  // the host n-gram writer: the fixture's lines in any order, and they load back as the model
  double seconds[4] = {0, 0, 0, 0};
  CHECK(sg::lm_store_google_host(lm, scratch.c_str(), seconds, err) == SG_OK);
  for (int k = 1; k <= 3; k++) CHECK(sorted_lines(scratch + "/" + std::to_string(k) + "-gm") == sorted_lines(golden + "/" + std::to_string(k) + "-gm"));
  sg::HostLM back;
  CHECK(sg::lm_load_google(scratch.c_str(), 3, "<S>", "</S>", alphabet, 0, back, err) == SG_OK);
  CHECK(back.words == lm.words);
  for (size_t k = 0; k < 3 && k < back.level.size(); k++)
    CHECK(back.level[k].word == lm.level[k].word && back.level[k].count == lm.level[k].count && back.level[k].child_begin == lm.level[k].child_begin);
  CHECK(sg::lm_store_google_host(lm, (scratch + "/no/such/dir").c_str(), seconds, err) == SG_E_INVALID);
  CHECK(err.find("no/such/dir/1-gm") != std::string::npos);

  // generated vocabularies around the sort's thresholds (12: insertion sort; 40: the ninther) and a large one
  for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)12, (size_t)13, (size_t)40, (size_t)41, (size_t)1000, (size_t)20000}) {
    std::vector<std::string> words;
    uint64_t x = 88172645463325252ull + n;
    for (size_t i = 0; i < n; i++) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      std::string w = i == 0 ? std::string("q") : i == 1 ? std::string(300, 'z') : std::string();
      for (uint64_t v = x, j = 0; w.empty() || (i > 1 && j < 2 + (x >> 60)); j++, v /= 26) w.push_back((char)('a' + v % 26));
      words.push_back(w + (i > 1 ? "_" + std::to_string(i) : ""));
    }
    std::vector<uint32_t> values;
    std::vector<int32_t> aux;
    CHECK(sg::mph_build(words, values, aux, err) == SG_OK);
    CHECK(values.size() == n && aux.size() == n);
    bool ok = true;
    for (size_t i = 0; i < n && ok; i++) ok = mph_get(values, aux, words[i]) == i;
    CHECK(ok);
    std::vector<uint32_t> perm(values);
    std::sort(perm.begin(), perm.end());
    for (size_t i = 0; i < n && ok; i++) ok = perm[i] == i;
    CHECK(ok);
  }
  {
    std::vector<uint32_t> values;
    std::vector<int32_t> aux;
    CHECK(sg::mph_build({"a", "b", "a"}, values, aux, err) == SG_E_UNSUPPORTED);
  }
  printf("%d passed, %d failed\n", passed, failed);
  return failed ? 1 : 0;
}
