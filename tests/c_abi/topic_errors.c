/* rdx_topic_boost's argument checks, which come before any HIP call and so need no GPU: a plain C program built with
 * -fsanitize=address,undefined by tests/test_topics.py. Every call must return RDX_ERR_INVALID with a message, touch none of the
 * (deliberately tiny) buffers, and leave the process alive. */
#include <stdio.h>

#include "rdx.h"

#define EXPECT_INVALID(call)                                                                   \
    do {                                                                                       \
        int rc_ = (call);                                                                      \
        if (rc_ != RDX_ERR_INVALID || rdx_last_error() == NULL || rdx_last_error()[0] == 0) {  \
            fprintf(stderr, "%s -> %d (wanted %d): %s\n", #call, rc_, RDX_ERR_INVALID, rdx_last_error()); \
            return 1;                                                                          \
        }                                                                                      \
        ++n_checked;                                                                           \
    } while (0)

int main(void) {
    int n_checked = 0;
    if (rdx_version() != RDX_ABI_VERSION) return 2;
    float table[8] = {1, 0, 0, 0, 0, 1, 0, 0};
    int32_t slots[2] = {0, 1}, offsets[2] = {0, 1};
    int32_t pairs[1] = {RDX_TOPIC_PAIR(0, 0, 0)};
    double sims[1], boosts[1], best[1];
    if (RDX_TOPIC_PAIR(31, 65535, 1) != ((65535 << 8) | 128 | 31) || RDX_TOPIC_PAIR(3, 2, 0) != ((2 << 8) | 3)) return 3;
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 0, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 1025, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 0, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4097, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 33, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, -1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 65537, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 2049, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, -1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, -1, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, NULL, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, NULL, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, NULL, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, offsets, NULL, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, NULL, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, (double*)((char*)best + 4), NULL));
    EXPECT_INVALID(rdx_topic_boost(0, table, 2, 4, slots, 1, (int32_t*)((char*)slots + 2), 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(64, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    EXPECT_INVALID(rdx_topic_boost(-1, table, 2, 4, slots, 1, slots + 1, 1, offsets, pairs, 1, 1, 0.65, 0.15, sims, boosts, best, NULL));
    printf("topic boost error paths ok: %d checks\n", n_checked);
    return 0;
}
