// The (user, item) pair layouts a kernel can be handed: a training batch (u, i, j) or one of the four scoring layouts.
// Used by NeuMF (neumf.hip) and NFM (nfm.hip).
#pragma once
#include "common.h"

namespace daisy {

// the three pair layouts of daisy_neumf_scores, "these users x all items" of daisy_neumf_scores_users, plus the training batch
struct PairSrc {
    const int32_t *u, *i, *j;     // training: row r < B -> (u[r], i[r]); r >= B -> (u[r-B], j[r-B])
    int64_t B;
    const int64_t *users, *items; // scoring
    int64_t C;                    // > 0: user of pair e = users[e / C];  0 with items == NULL: (users[0], e)
    int64_t base;                 // first pair of this chunk
    int64_t all_items;            // > 0: pair e = (users[e / all_items], e % all_items) - no candidate array exists
};
__device__ __forceinline__ void pair_ids(const PairSrc &s, int64_t r, int64_t &user, int64_t &item) {
    if (s.u) {
        const int64_t b = (r < s.B) ? r : r - s.B;
        user = s.u[b];
        item = (r < s.B) ? s.i[b] : s.j[b];
    } else {
        const int64_t e = s.base + r;
        if (s.all_items > 0) { user = s.users[e / s.all_items]; item = e % s.all_items; }
        else if (!s.items) { user = s.users[0]; item = e; }
        else if (s.C > 0) { user = s.users[e / s.C]; item = s.items[e]; }
        else { user = s.users[e]; item = s.items[e]; }
    }
}

}  // namespace daisy
