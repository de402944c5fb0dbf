// d1_graft_sanitized.cpp — the grafting of host/cluster_d1.cpp under AddressSanitizer and UBSan, as a program of its own: no
// GPU, no Python.  A hand-made clustering of 40 amplicons in 20 swarms is grafted three ways — swa_d1_graft from candidates,
// swa_d1_result_install_graft on a result with its details on the host, and on a prepared (pinned) lazy result —; -o -s -i -u
// must be the same files, refusals must change nothing, and the pinned member order must be unpinned once, as the pointer it
// was pinned as.  What checks the move of the member order for accesses out of bounds is the sanitizer.  The thirteen calls
// into the device library that cluster_d1.cpp links are stubs here (the clustering's download and the details' among them).
//   make -C swarm_amd/csrc graft-check
#include "swarm_amd_host.h"
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <filesystem>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

static const std::vector<uint32_t> kSizes = {6, 5, 4, 3, 2, 2, 1, 1, 1, 3, 1, 2, 1, 1, 1, 2, 1, 1, 1, 1};   // 40 amplicons, 20 swarms
static const uint32_t kHeavy = 3;                                      // the first three swarms are heavy
static int g_pins = 0, g_unpins = 0;
static void * g_pinned = nullptr;

extern "C" {
const char * swa_last_error(const swa_ctx *) { return "stub"; }
int swa_host_pin(swa_ctx *, void * p, size_t) { ++g_pins; g_pinned = p; return SWA_OK; }
void swa_host_unpin(void * p) { ++g_unpins; if (p != g_pinned) { std::fprintf(stderr, "unpin of another pointer\n"); std::abort(); } }
int swa_d1_cluster_device(swa_ctx *, uint32_t *, uint32_t *, uint32_t *, uint32_t * order, uint32_t * begin, uint32_t cap, uint32_t * nswarms) {
  uint32_t at = 0;
  for (size_t s = 0; s < kSizes.size(); ++s) { begin[s] = at; for (uint32_t k = 0; k < kSizes[s]; ++k) { order[at] = at; ++at; } }
  begin[kSizes.size()] = at;
  (void)cap;
  *nswarms = (uint32_t)kSizes.size();
  return SWA_OK;
}
int swa_d1_cluster_fetch(swa_ctx *, uint32_t * sid, uint32_t * gen, uint32_t * par) {
  uint32_t at = 0;
  for (size_t s = 0; s < kSizes.size(); ++s) {
    const uint32_t seed = at;
    for (uint32_t k = 0; k < kSizes[s]; ++k, ++at) { sid[at] = (uint32_t)s; gen[at] = k == 0 ? 0 : 1; par[at] = k == 0 ? SWA_NO_AMPLICON : seed; }
  }
  return SWA_OK;
}
uint32_t swa_d1_cluster_maxgen(const swa_ctx *) { return 1; }
int swa_d1_graft_candidates_fetch(swa_ctx *, uint32_t *) { return SWA_E_ARG; }
int swa_d1_graft_layout_device(swa_ctx *, uint32_t *, uint32_t *, uint32_t *, uint8_t *, uint32_t, uint64_t *) { return SWA_E_ARG; }
int swa_d1_graft_layout_info(const swa_ctx *, uint64_t * o) { o[0] = 0; return SWA_OK; }
int swa_nw_batch(swa_ctx *, uint64_t, uint64_t, uint64_t, uint64_t, const uint32_t *, const uint32_t *, uint32_t *, uint32_t *, uint64_t *, char *, uint64_t, uint64_t *) { return SWA_E_ARG; }
int swa_nw_batch_totals(const swa_ctx *, uint64_t *) { return SWA_E_ARG; }
int swa_nw_batch_tiers(const swa_ctx *, uint64_t *) { return SWA_E_ARG; }
int swa_nw_batch_text_full(const swa_ctx *, uint64_t *) { return SWA_E_ARG; }
}

static std::string slurp(const std::string & p) { std::ifstream f(p); std::stringstream s; s << f.rdbuf(); return s.str(); }
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
  const uint32_t n = 40;
  char made[] = "/tmp/d1_graft_XXXXXX";
  CHECK(mkdtemp(made) != nullptr);
  const std::string dir = std::string(made) + "/";
  // FASTA: abundance falls along the ids (9 for members of heavy swarms, 1 for the rest), headers ascend
  {
    std::ofstream f(dir + "in.fa");
    uint32_t at = 0;
    srand(7);
    for (size_t s = 0; s < kSizes.size(); ++s) {
      for (uint32_t k = 0; k < kSizes[s]; ++k, ++at) {
        char h[32];
        std::snprintf(h, sizeof h, "a%06u_%u", at, s < kHeavy ? 9u : 1u);
        std::string seq;
        for (int j = 0; j < 40; ++j) { seq += "ACGT"[rand() & 3]; }
        f << '>' << h << '\n' << seq << '\n';
      }
    }
  }
  swa_hostdb * db = nullptr;
  CHECK(swa_hostdb_read_fasta((dir + "in.fa").c_str(), 0, 0, 0, &db) == SWA_OK);
  // CSR: every seed links to the other members of its block
  std::vector<uint64_t> off(n + 1, 0);
  std::vector<uint32_t> nb, begins;
  {
    uint32_t at = 0;
    for (size_t s = 0; s < kSizes.size(); ++s) {
      begins.push_back(at);
      for (uint32_t k = 0; k < kSizes[s]; ++k) {
        if (k == 0) { for (uint32_t j = 1; j < kSizes[s]; ++j) { nb.push_back(at + j); } }
        off[at + k + 1] = nb.size();
      }
      at += kSizes[s];
    }
    begins.push_back(at);
  }
  // candidates: light swarm s hangs on heavy swarm s % 3 (a later member of it); two children in swarm 9 (one is withdrawn);
  // swarm 11 has none
  std::vector<uint32_t> cand(n, SWA_NO_AMPLICON);
  for (uint32_t s = kHeavy; s < kSizes.size(); ++s) {
    if (s == 11) { continue; }
    const uint32_t h = s % kHeavy;
    cand[begins[s]] = begins[h] + (s % kSizes[h]);
  }
  cand[begins[9] + 2] = begins[0];
  // the grafts in chain order, for the install
  std::vector<uint32_t> sid(n);
  for (size_t s = 0; s < kSizes.size(); ++s) { for (uint32_t k = begins[s]; k < begins[s + 1]; ++k) { sid[k] = (uint32_t)s; } }
  std::vector<uint64_t> pairs;
  for (uint32_t i = 0; i < n; ++i) { if (cand[i] != SWA_NO_AMPLICON) { pairs.push_back(((uint64_t)cand[i] << 32) | i); } }
  std::sort(pairs.begin(), pairs.end());
  std::vector<bool> taken(kSizes.size(), false);
  std::vector<std::pair<uint64_t, uint64_t>> wins;                       // (heavy << 32 | rank, pair)
  for (uint64_t p : pairs) {
    const uint32_t l = sid[(uint32_t)p];
    if (taken[l]) { continue; }
    taken[l] = true;
    wins.push_back({((uint64_t)sid[p >> 32] << 32) | wins.size(), p});
  }
  std::sort(wins.begin(), wins.end());
  std::vector<uint32_t> heavy, light, parent, child;
  for (auto & w : wins) { heavy.push_back((uint32_t)(w.first >> 32)); parent.push_back((uint32_t)(w.second >> 32)); child.push_back((uint32_t)w.second); light.push_back(sid[child.back()]); }
  const uint32_t G = (uint32_t)wins.size();
  CHECK(G == 16);

  // route 1
  swa_d1_result * a = nullptr;
  CHECK(swa_d1_cluster(db, off.data(), nb.data(), &a) == SWA_OK);
  uint64_t before[4], after[4];
  swa_d1_result_summary(a, before);
  {  // ill-formed: swarm 11 hangs on a member of swarm 12, which is won itself
    std::vector<uint32_t> ill = cand;
    ill[begins[11]] = begins[12];
    CHECK(swa_d1_graft(a, ill.data()) == 0);
    swa_d1_result_summary(a, after);
    CHECK(std::memcmp(before, after, sizeof before) == 0 && swa_d1_result_graft_route(a) == 0 && std::strlen(swa_d1_result_error(a)) > 0);
    ill = cand;
    ill[5] = n + 3;                                                       // no amplicon
    CHECK(swa_d1_graft(a, ill.data()) == 0 && swa_d1_result_graft_route(a) == 0);
  }
  CHECK(swa_d1_graft(a, cand.data()) == G && swa_d1_result_graft_route(a) == 1);
  CHECK(swa_d1_graft(a, cand.data()) == 0);                               // grafts on top of grafts
  CHECK(swa_d1_write_swarms(a, db, (dir + "a.o").c_str(), 0, 0, 0, 1) == SWA_OK);
  CHECK(swa_d1_write_stats(a, db, (dir + "a.s").c_str(), 0) == SWA_OK);
  CHECK(swa_d1_write_structure(a, db, (dir + "a.i").c_str(), 0) == SWA_OK);
  CHECK(swa_d1_write_uclust(a, db, (dir + "a.u").c_str(), 0, 0, 18, 24, 13) == SWA_OK);
  // route 2, details on the host
  swa_d1_result * b = nullptr;
  CHECK(swa_d1_cluster(db, off.data(), nb.data(), &b) == SWA_OK);
  {  // refusals change nothing
    std::vector<uint32_t> h2 = heavy, l2 = light;
    l2[3] = l2[2];
    CHECK(swa_d1_result_install_graft(b, h2.data(), l2.data(), parent.data(), child.data(), G) == SWA_E_ARG);
    h2[5] = 400;
    CHECK(swa_d1_result_install_graft(b, h2.data(), light.data(), parent.data(), child.data(), G) == SWA_E_ARG);
    h2 = heavy; std::swap(h2[0], h2[G - 1]);
    CHECK(swa_d1_result_install_graft(b, h2.data(), light.data(), parent.data(), child.data(), G) == SWA_E_ARG);
    swa_d1_result_summary(b, after);
    CHECK(std::memcmp(before, after, sizeof before) == 0 && swa_d1_result_graft_route(b) == 0);
  }
  CHECK(swa_d1_result_install_graft(b, heavy.data(), light.data(), parent.data(), child.data(), G) == SWA_OK);
  CHECK(swa_d1_write_swarms(b, db, (dir + "b.o").c_str(), 0, 0, 0, 1) == SWA_OK);
  CHECK(swa_d1_write_stats(b, db, (dir + "b.s").c_str(), 0) == SWA_OK);
  CHECK(swa_d1_write_structure(b, db, (dir + "b.i").c_str(), 0) == SWA_OK);
  CHECK(swa_d1_write_uclust(b, db, (dir + "b.u").c_str(), 0, 0, 18, 24, 13) == SWA_OK);
  // route 2 on a prepared (pinned), lazy result: -o before the details, -s -i after
  swa_ctx * ctx = reinterpret_cast<swa_ctx *>(&g_pins);                  // (never dereferenced: every call on it is a stub)
  swa_d1_result * c = nullptr;
  CHECK(swa_d1_result_prepare(ctx, db, &c) == SWA_OK && g_pins == 1);
  CHECK(swa_d1_cluster_resident_prepared(ctx, db, c) == SWA_OK);
  CHECK(swa_d1_result_install_graft(c, heavy.data(), light.data(), parent.data(), child.data(), G) == SWA_OK);
  CHECK(swa_d1_write_swarms(c, db, (dir + "c.o").c_str(), 0, 0, 0, 1) == SWA_OK && swa_d1_result_detail_fetches(c) == 0);
  CHECK(swa_d1_write_stats(c, db, (dir + "c.s").c_str(), 0) == SWA_OK && swa_d1_result_detail_fetches(c) == 1);
  CHECK(swa_d1_write_structure(c, db, (dir + "c.i").c_str(), 0) == SWA_OK);
  CHECK(swa_d1_write_uclust(c, db, (dir + "c.u").c_str(), 0, 0, 18, 24, 13) == SWA_OK);
  for (const char * k : {"o", "s", "i", "u"}) {
    const std::string x = slurp(dir + "a." + k);
    CHECK(!x.empty() && x == slurp(dir + "b." + k) && x == slurp(dir + "c." + k));
  }
  swa_d1_result_summary(a, before);
  swa_d1_result_summary(b, after);
  CHECK(std::memcmp(before, after, sizeof before) == 0);
  swa_d1_result_summary(c, after);
  CHECK(std::memcmp(before, after, sizeof before) == 0 && before[0] == kSizes.size() - G);
  swa_d1_result_free(a);
  swa_d1_result_free(b);
  CHECK(g_unpins == 0);
  swa_d1_result_free(c);
  CHECK(g_pins == 1 && g_unpins == 1);
  swa_hostdb_free(db);
  std::filesystem::remove_all(made);
  std::printf("ok: %u grafts, three routes, files equal, pinned once and unpinned once\n", G);
  return 0;
}
