// mixed_load — single_query_load's calling pattern (one blocking sg_suggest_one per thread, many threads) with traffic that does
// NOT share one set of search parameters: thread t asks under key t % keys.  With sg_coalesce_mixed off every take of the
// dispatcher serves one key; on, a take with several keys is ONE mixed call.  Every answer is checked against the rows of one
// sg_suggest_batch call per key over the same queries.
// A program of its own beside single_query_load.cpp, which stays as it is: the synthesis of the dictionary and of the queries
// (mix() and the loops that use it) is therefore stated in both files — a change to one belongs in the other too.
//   usage: mixed_load <dict_size> <threads> <seconds> <keys 1..8> <mixed 0|1>   -> one JSON line
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/suggest_hip.h"

static uint64_t mix(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return x;
}

struct Key { int metric; double sim; uint32_t k; };
// the BASELINE configs' parameters and neighbours of them
static const Key kKeys[8] = {{SG_JACCARD, 0.5, 10}, {SG_COSINE, 0.4, 20}, {SG_DICE, 0.5, 10}, {SG_JACCARD, 0.6, 5},
                             {SG_COSINE, 0.5, 10}, {SG_DICE, 0.6, 20}, {SG_JACCARD, 0.4, 10}, {SG_OVERLAP, 0.7, 10}};

int main(int argc, char** argv) {
  const uint32_t n_docs = argc > 1 ? (uint32_t)atoi(argv[1]) : 1000000u;
  const int n_thr = argc > 2 ? atoi(argv[2]) : 256;
  const double secs = argc > 3 ? atof(argv[3]) : 3.0;
  const int n_keys = argc > 4 ? atoi(argv[4]) : 2;
  const int mixed = argc > 5 ? atoi(argv[5]) : 0;
  if (n_keys < 1 || n_keys > 8 || n_thr < 1) { fprintf(stderr, "keys 1..8, threads >= 1\n"); return 2; }
  const uint32_t n_q = 16384;
  const char* sym = "abcdefghijklmnopqrstuvwxyz0123456789";
  std::string blob;
  std::vector<uint64_t> offs(1, 0);
  for (uint32_t d = 0; d < n_docs; d++) {
    const uint32_t len = 8 + (uint32_t)(mix(d * 2654435761ull + 1) % 25);
    for (uint32_t c = 0; c < len; c++) blob.push_back(sym[mix(((uint64_t)d << 8) + c + 77) % 36]);
    offs.push_back(blob.size());
  }
  std::string qblob;
  std::vector<uint64_t> qoffs(1, 0);
  for (uint32_t q = 0; q < n_q; q++) {                       // a dictionary string with one substitution
    const uint32_t d = (uint32_t)(mix(q + 0x1234567ull) % n_docs);
    std::string s = blob.substr(offs[d], offs[d + 1] - offs[d]);
    s[mix(q * 31 + 5) % s.size()] = sym[mix(q * 17 + 3) % 36];
    qblob += s;
    qoffs.push_back(qblob.size());
  }
  const char* alpha[] = {"english", "numbers", "$"};
  sg_desc desc{3, "$", "$", "$", alpha, 3};
  sg_index* ix = nullptr;
  if (sg_index_build_device((const uint8_t*)blob.data(), offs.data(), n_docs, &desc, 0, &ix) || sg_index_upload(ix, 0)) {
    fprintf(stderr, "build/upload failed: %s\n", sg_last_error());
    return 2;
  }
  std::vector<std::vector<uint32_t>> ids(n_keys), cnt(n_keys);
  std::vector<std::vector<double>> sc(n_keys);
  for (int g = 0; g < n_keys; g++) {
    const Key& key = kKeys[g];
    ids[g].resize((size_t)n_q * key.k); sc[g].resize((size_t)n_q * key.k); cnt[g].resize(n_q);
    if (sg_suggest_batch(ix, (const uint8_t*)qblob.data(), qoffs.data(), n_q, key.metric, key.sim, key.k, ids[g].data(), sc[g].data(), cnt[g].data())) {
      fprintf(stderr, "batch failed: %s\n", sg_last_error());
      return 2;
    }
  }
  if (sg_coalesce_mixed(ix, mixed)) { fprintf(stderr, "sg_coalesce_mixed: %s\n", sg_last_error()); return 2; }
  uint64_t st0[4] = {0, 0, 0, 0}, st1[4] = {0, 0, 0, 0};
  sg_debug_coalesce_stats(ix, st0);
  std::atomic<uint64_t> done{0}, bad{0};
  std::atomic<bool> stop{false};
  std::vector<std::thread> pool;
  const auto t0 = std::chrono::steady_clock::now();
  for (int t = 0; t < n_thr; t++)
    pool.emplace_back([&, t] {
      const int g = t % n_keys;
      const Key& key = kKeys[g];
      uint32_t my_ids[32]; double my_sc[32]; uint32_t my_cnt = 0;
      uint64_t n = 0, wrong = 0;
      for (uint32_t q = (uint32_t)t % n_q; !stop.load(std::memory_order_relaxed); q = (q + (uint32_t)n_thr) % n_q) {
        const int rc = sg_suggest_one(ix, (const uint8_t*)qblob.data() + qoffs[q], (uint32_t)(qoffs[q + 1] - qoffs[q]), key.metric, key.sim, key.k,
                                      my_ids, my_sc, &my_cnt);
        bool ok = rc == 0 && my_cnt == cnt[g][q];
        for (uint32_t j = 0; ok && j < my_cnt && j < key.k; j++)
          ok = my_ids[j] == ids[g][(size_t)q * key.k + j] && memcmp(&my_sc[j], &sc[g][(size_t)q * key.k + j], 8) == 0;
        if (!ok && bad.load() + wrong < 6) fprintf(stderr, "mismatch q=%u key=%d rc=%d cnt %u vs %u\n", q, g, rc, my_cnt, cnt[g][q]);
        wrong += !ok;
        n++;
      }
      done += n; bad += wrong;
    });
  std::this_thread::sleep_for(std::chrono::duration<double>(secs));
  stop = true;
  for (auto& th : pool) th.join();
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  sg_debug_coalesce_stats(ix, st1);
  const uint64_t batches = st1[1] - st0[1], mixed_batches = st1[2] - st0[2], launches = st1[3] - st0[3];
  printf("{\"dict\": %u, \"threads\": %d, \"keys\": %d, \"mixed\": %d, \"seconds\": %.3f, \"queries\": %llu, \"qps\": %.0f, \"batches\": %llu, "
         "\"mixed_batches\": %llu, \"launches\": %llu, \"queries_per_batch\": %.1f, \"mismatches\": %llu}\n",
         n_docs, n_thr, n_keys, mixed, dt, (unsigned long long)done.load(), (double)done.load() / dt, (unsigned long long)batches,
         (unsigned long long)mixed_batches, (unsigned long long)launches, batches ? (double)done.load() / (double)batches : 0.0,
         (unsigned long long)bad.load());
  sg_index_release(ix);
  return bad.load() ? 1 : 0;
}
