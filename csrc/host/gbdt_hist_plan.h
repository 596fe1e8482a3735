// The histogram task lists of the GBDT growers (csrc/bind/gbdt_ops.cc) for
// row segments whose lengths the host knows (or bounds): gbdt.hip k_hist
// runs one block per task, k_hist_reduce sums a segment's chunk partials.
// Free of HIP and torch: the binding and the host self-test compile the same
// code.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace wh {

// Appends to `tasks` (int32 x 5) and `red` (int32 x 6). Segment k of length
// seglen[k] is cut into nch = max(1, ceil(len / chunk)) chunks (an empty
// segment keeps one, so its histogram is still written):
//   tasks, chunk-major then feature group: {k, fbeg, fcnt, c, chunk}
//   red, one per feature group gi:         {k, fbeg, fcnt, t0 + gi, nch, G}
// where t0 is the segment's first task and G the number of groups, so a
// reduce record reads tasks t0 + gi, t0 + gi + G, ... (nch of them).
inline void gbdt_hist_plan(const std::vector<int64_t>& seglen,
                           const std::vector<std::pair<int64_t, int64_t>>& fgroups, int chunk,
                           std::vector<int32_t>* tasks, std::vector<int32_t>* red) {
  const int G = (int)fgroups.size();
  for (int k = 0; k < (int)seglen.size(); ++k) {
    const int64_t nch = std::max<int64_t>(1, (seglen[k] + chunk - 1) / chunk);
    const int t0 = (int)(tasks->size() / 5);
    for (int64_t c = 0; c < nch; ++c)
      for (auto& fg : fgroups)
        tasks->insert(tasks->end(), {k, (int)fg.first, (int)fg.second, (int)c, chunk});
    for (int gi = 0; gi < G; ++gi)
      red->insert(red->end(), {k, (int)fgroups[gi].first, (int)fgroups[gi].second, t0 + gi,
                               (int)nch, G});
  }
}

}  // namespace wh
