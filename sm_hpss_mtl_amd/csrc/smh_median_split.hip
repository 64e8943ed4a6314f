// Instantiations of the block-split median kernel (windows up to 21): smh_median_split.h, from the lists of smh_median_plan.h.
#include "smh_median_split.h"

namespace smh_median {

SplitFn find_split_kernel(int lh, int lp, bool dma) {
#define SMH_SPLIT_E2(a, b) \
    if (lh == a && lp == b) return !dma ? hpss_median_split_kernel<a, b> : hpss_median_split_kernel<a, b, true>;
#define SMH_SPLIT_SINGLE(w) SMH_SPLIT_E2(w, 0) SMH_SPLIT_E2(0, w)
    SMH_MEDIAN_SPLIT_PAIRS(SMH_SPLIT_E2)
    SMH_MEDIAN_SPLIT_SINGLES(SMH_SPLIT_SINGLE)
    return nullptr;
}

PersistFn find_persist_kernel(int lh, int lp, int threads) {
#define SMH_PERSIST_E3(a, b, t) \
    if (lh == a && lp == b && threads == t) return hpss_median_persist_kernel<a, b, t>;
    SMH_MEDIAN_PERSIST_BUILDS(SMH_PERSIST_E3)
    return nullptr;
}

}  // namespace smh_median
