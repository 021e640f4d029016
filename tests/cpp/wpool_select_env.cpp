// The wave pool's instance selection over the environment half of its request space
// (cvr_wpool_select.h: requests kWpoolRequests .. kWpoolRequestsAll - 1), one line per request
// (tests/test_wpool_select_env.py checks them against the rule cvr.h states):
//   scatter_eps waves sparse full uniform half naive_mk count_words moments record flush env : eps waves med record flush
// or `-` after the colon where no instance runs the request.
#include <cstdio>

#include "cvr_wpool_select.h"

int main() {
  static_assert(cvr::kWpoolRequestsAll == 2 * cvr::kWpoolRequests, "the environment half follows the plain one");
  for (int i = cvr::kWpoolRequests; i < cvr::kWpoolRequestsAll; ++i) {
    const cvr::WpoolRequest q = cvr::wpool_request_at(i);
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d :", q.scatter_eps, q.waves, q.sparse, q.full, q.uniform, q.half,
                q.naive_mk, q.count_words, q.moments, q.record, q.flush, q.env);
    cvr::WpoolInstance k{};
    if (cvr::wpool_select(q, &k))
      std::printf(" %d %d %d %d %d\n", k.eps, k.waves, k.med, k.record, k.flush);
    else
      std::printf(" -\n");
  }
  return 0;
}
