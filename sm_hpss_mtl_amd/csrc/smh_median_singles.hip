// Single-filter instantiations (any odd window 3..63) of the HPSS median kernel, from the list of smh_median_plan.h.
#include "smh_median_kernel.h"

namespace smh_median {

KernelFn find_single_kernel(int lh, int lp) {
#define SMH_MEDIAN_SINGLE(w)                                    \
    if (lh == w && lp == 0) return hpss_median_kernel<w, 0>; \
    if (lh == 0 && lp == w) return hpss_median_kernel<0, w>;
    SMH_MEDIAN_SINGLES(SMH_MEDIAN_SINGLE)
    return nullptr;
}

}  // namespace smh_median
