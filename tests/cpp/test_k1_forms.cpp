// The K1 kernels are instantiated per form (FAST or general) and the host picks one per launch.  This
// program plans launches through k1_plan on both sides of 2^33 and 2^40 and checks that the instantiation
// picked is the one the launch-uniform flag selected when one kernel held both bodies:
//   FAST  <=>  (lo >> 33) == ((hi - 1) >> 33)  &&  hi <= 2^40
// A stand-alone program that makes no GPU call: the translation unit of the element kernels is included
// whole, so the planner and the kernels' host stubs are the product's.  It is built as an ordinary HIP
// program, device code included (a host-only build leaves the fat binary's symbol undefined at link time);
// only the host code is built with the sanitizers.
#include <cstdio>
#include <cstdlib>

#include "rsv_elements.hip"

using namespace rsv;

static int checked = 0;

static void check(uint32_t k, uint64_t lo, uint64_t n, bool want_fast) {
    const uint64_t hi = lo + n, g_begin = lo >> 4, n_groups = ((hi + 15) >> 4) - g_begin;
    // one launch: no crossing of a multiple of 2^32 blocks, fewer than 2^31 blocks (launch_k1_last_writer's split)
    if (n_groups > (1ull << 31) || ((hi + 15) >> 4) > (((g_begin >> 32) + 1) << 32)) {
        printf("case (%llu, %llu) is not one launch\n", (unsigned long long)lo, (unsigned long long)n);
        exit(1);
    }
    K1Launch P;
    const unsigned grid = k1_plan(k, lo, hi, g_begin, n_groups, P);
    const bool rule = (lo >> 33) == ((hi - 1) >> 33) && hi <= (1ull << 40);
    const bool flag = (P.flags & kK1Fast) != 0;
    const bool kernel_fast = k1_last_writer_for(P) == k1_last_writer<true>;
    const bool kernel_general = k1_last_writer_for(P) == k1_last_writer<false>;
    const bool fused_l = k1_resolve_publish_for<int64_t>(P) == k1_resolve_publish<int64_t, true>;
    const bool fused_l_general = k1_resolve_publish_for<int64_t>(P) == k1_resolve_publish<int64_t, false>;
    const bool fused_i = k1_resolve_publish_for<int32_t>(P) == k1_resolve_publish<int32_t, true>;
    const bool fused_i_general = k1_resolve_publish_for<int32_t>(P) == k1_resolve_publish<int32_t, false>;
    const bool ok = grid > 0 && rule == want_fast && flag == want_fast && kernel_fast == want_fast &&
                    kernel_general == !want_fast && fused_l == want_fast && fused_l_general == !want_fast &&
                    fused_i == want_fast && fused_i_general == !want_fast;
    if (!ok) {
        printf("lo %llu n %llu: want %d rule %d flag %d kernel %d/%d fused %d/%d %d/%d grid %u\n", (unsigned long long)lo,
               (unsigned long long)n, want_fast, rule, flag, kernel_fast, kernel_general, fused_l, fused_l_general, fused_i,
               fused_i_general, grid);
        exit(1);
    }
    ++checked;
}

int main() {
    const uint64_t p33 = 1ull << 33, p36 = 1ull << 36, p40 = 1ull << 40, N9 = 1000000000ull, N8 = 80000003ull;
    for (uint32_t k : {1u, 1024u, 2048u, 1u << 20}) {
        check(k, 0, N9 + 7, true);                // the schedule from index 0
        check(k, 5, 1ull << 27, true);            // the fused form's size
        check(k, p33 - N9, N9, true);             // ends at 2^33: the last index is below it
        check(k, p33 - N9, N9 + 1, false);        // index 2^33 is in: the level-1 high word is not uniform
        check(k, p33 - 1, N8, false);
        check(k, p33, N9, true);                  // starts at 2^33
        check(k, 3 * p33 - N9 / 2 - 9, N9, false);
        check(k, p36 + 5, N8, true);              // block counter high word 1
        check(k, p36 + 5, N9, true);
        check(k, p40 - 40000000ull, 40000000ull, true);       // ends at 2^40: every index below it
        check(k, p40 - 8 * N9, 8 * N9, true);                 // a 2^31-block-sized launch up to 2^40
        check(k, p40, N8, false);                 // from 2^40: hi-uniform, not below 2^40
        check(k, p40 + 3, N8, false);
        check(k, p40 + 3, N9, false);
        check(k, 5 * p40 + p33 - N8 / 2, N8, false);  // past 2^40 and across a multiple of 2^33
    }
    printf("ok %d\n", checked);
    return 0;
}
