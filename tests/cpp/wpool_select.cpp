// The wave pool's instance selection over its whole request space, one line per request
// (tests/test_wpool_select.py compares them with tests/golden/wpool_instances.txt):
//   scatter_eps waves sparse full uniform half naive_mk count_words moments record flush : eps waves med record flush
// or `-` after the colon where no instance runs the request.
#include <cstdio>

#include "cvr_wpool_select.h"

int main() {
  for (int i = 0; i < cvr::kWpoolRequests; ++i) {
    const cvr::WpoolRequest q = cvr::wpool_request_at(i);
    std::printf("%d %d %d %d %d %d %d %d %d %d %d :", q.scatter_eps, q.waves, q.sparse, q.full, q.uniform, q.half,
                q.naive_mk, q.count_words, q.moments, q.record, q.flush);
    cvr::WpoolInstance k{};
    if (cvr::wpool_select(q, &k))
      std::printf(" %d %d %d %d %d\n", k.eps, k.waves, k.med, k.record, k.flush);
    else
      std::printf(" -\n");
  }
  return 0;
}
