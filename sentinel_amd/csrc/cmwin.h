// cmwin.h -- which bucket of a token server window counts at `now`: the one predicate that the decision path's sums
// (cluster.hip cm_sum) and the metrics read-back (cmetrics.hip) share.
#pragma once

// A bucket that was never created (start < 0), or that LeapArray.isWindowDeprecated drops (now - start > interval,
// strict), adds nothing to a sum at now.  A macro, so that `interval` is read only for a bucket that exists, as
// cm_sum always did: its kernels compile to the code they had before the predicate moved here.
#define CM_SKIPPED(start, now, interval) ((start) < 0 || (now) - (start) > (interval))
