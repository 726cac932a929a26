// hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/devprep_carve_check.hip score_amd/csrc/sort.hip -o /tmp/devprep_carve_check && /tmp/devprep_carve_check
//
// The nine workspace layouts of the device data builds and of the history exclusions (csrc/devprep.h's Carver) on the host, no GPU: each is carved with a null
// base (sizes only: every pointer must stay null) and over a malloc of exactly that size (every range inside the block, one
// behind the other, and written to, so the sanitizer sees a range that leaves the block).  The six files are included as they
// are, each in a namespace of its own; the sizes are also held against the public *_temp_bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Seen { char* p; long long bytes; };
static std::vector<Seen> g_seen;
#define DP_CARVE_SEEN(p, bytes) g_seen.push_back(Seen{reinterpret_cast<char*>(p), (long long)(bytes)})

#include "../score_amd/csrc/cellkey.h"
#include "../score_amd/csrc/devprep.h"
namespace ph {
#include "../score_amd/csrc/pointhist.hip"
}
namespace gb {
#include "../score_amd/csrc/graphbuild.hip"
}
namespace tg {
#include "../score_amd/csrc/targetgen.hip"
}
namespace lr {
#include "../score_amd/csrc/logremap.hip"
}
namespace cc {
#include "../score_amd/csrc/ccmr.hip"
}
namespace hx {
#include "../score_amd/csrc/histexcl.hip"
}

static int g_failed = 0;

template <class F>
static void check(const char* name, long long n, int64_t want, F carve) {
  const auto fail = [&](const char* what) { std::printf("FAIL %s n=%lld: %s\n", name, n, what); ++g_failed; };
  g_seen.clear();
  const int64_t total = carve(nullptr);
  const std::vector<Seen> sizes = g_seen;
  for (const Seen& s : sizes)
    if (s.p) fail("a pointer from a null base");
  if (total != want || total <= 0) return fail("the size is not the public *_temp_bytes");
  char* block = static_cast<char*>(std::malloc((size_t)total));
  g_seen.clear();
  if (carve(block) != total || g_seen.size() != sizes.size()) fail("the second carve differs from the first");
  char* end = block;
  for (size_t i = 0; i < g_seen.size(); ++i) {
    const Seen& s = g_seen[i];
    if (s.bytes != sizes[i].bytes) fail("a range's size depends on the base");
    if (!s.p || s.p < end || s.bytes < 0 || s.p + s.bytes > block + total) { fail("a range overlaps the one before or leaves the block"); break; }
    std::memset(s.p, 0x5A, (size_t)s.bytes);
    end = s.p + s.bytes;
  }
  if (end != block + total) fail("the ranges do not fill the block");
  std::free(block);
  std::printf("ok   %-18s n=%-8lld %zu ranges, %lld bytes\n", name, n, sizes.size(), (long long)total);
}

int main() {
  for (const int64_t n : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)4097, (int64_t)1000003}) {
    const int32_t U = (int32_t)(n % 5000) + 3, I = (int32_t)(n % 70001) + 1, S = 11;
    const int64_t ncell = (int64_t)(U > I ? U : I) * S;
    if (n > 0) {
      check("score_point_hist", n, score_point_hist_temp_bytes(n), [&](void* t) { return ph::carve(t, n).total_bytes; });
      check("score_graph_build", n, score_graph_build_temp_bytes(n, U, I, S), [&](void* t) { return gb::carve(t, n, ncell).total_bytes; });
      check("score_target_build", n, score_target_build_temp_bytes(n, U), [&](void* t) { return tg::carve(t, n, U).total_bytes; });
      check("score_pop_items", n, score_pop_items_temp_bytes((int32_t)n), [&](void* t) { return tg::pop_carve(t, n).total_bytes; });
      check("score_log_remap", n, score_log_remap_temp_bytes(n, 3), [&](void* t) { return lr::carve(t, n).total_bytes; });
      check("score_log_compact", n, score_log_compact_temp_bytes(n), [&](void* t) { return lr::compact_carve(t, n).total_bytes; });
    }
    check("score_ccmr_prep", n, score_ccmr_prep_temp_bytes(n, I), [&](void* t) { return cc::prep_carve(t, n, I).total_bytes; });
    check("score_neg_lists", n, score_neg_lists_temp_bytes(n), [&](void* t) { return cc::neg_carve(t, n).total_bytes; });
    if (n > 0) {      // L = n lines against a catalogue of I items: n * ceil(I / range) counts
      int32_t nr = 0;
      int64_t want = -1;
      const int rc = score_catalog_history_exclusions_plan((int32_t)n, I, 0, nullptr, &nr, nullptr, &want);
      check("score_catalog_history_exclusions", n, rc == 0 ? want : -1, [&](void* t) { return hx::excl_carve(t, n * nr).total_bytes; });
    }
  }
  std::printf(g_failed ? "%d FAILED\n" : "all layouts hold\n", g_failed);
  return g_failed ? 1 : 0;
}
