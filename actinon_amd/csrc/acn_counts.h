/* acn_counts.h -- the counter blocks of a chunk: the only thing the device tells the pipeline runner.  The words of a level's block,
 * the ACN_FLAG_* bits of its flag word and the constants that size it, defined ONCE for the kernels that write them (acn_queues.h and the family headers,
 * acn_device.h), for the host planner that reads them (acn_queueplan.h: acn_read_chunk, acn_sample_rates) and for the tests.  Plain C,
 * valid as C99 and as C++, no HIP header: tests/csrc/chunkplan_cpu.c compiles the planner as C. */
#ifndef ACN_COUNTS_H
#define ACN_COUNTS_H

#define ACN_MAX_PATH_LEVELS 5    /* suspended path loops: trace_depth <= 10 * 5 + 10 */
#define ACN_LEVEL_BLOCKS ( ACN_MAX_PATH_LEVELS + 1 )   /* counter blocks of a chunk: one per path level */

/* the flag word of a chunk (QC_FLAGS of its first block; the host ORs the levels') */
#define ACN_FLAG_TASK_OVERFLOW  1u
#define ACN_FLAG_CHILD_OVERFLOW 2u
#define ACN_FLAG_STACK_OVERFLOW 4u   /* CSG / compound / ray stack exhausted: the result would be wrong, the call fails */
#define ACN_FLAG_CLAMPED        8u   /* a single pixel contribution exceeded the fixed-point clamp (reported, not an error) */
/* a queue overflowed: the chunk is lost, the host redoes it smaller and every later kernel of its chain leaves at once */
#define ACN_FLAGS_CHUNK_LOST ( ACN_FLAG_TASK_OVERFLOW | ACN_FLAG_CHILD_OVERFLOW )

#define ACN_NCLASS 4
/* One counter block per path level (uint32 each), all blocks of a chunk zeroed by one memset before its first launch.
 * Queue counters are high-water marks of reserved slots (dead slots included); QS_* are exact statistics.
 * QC_GEN + g: rays waiting for walk pass g of the level (g = 0: filled by k_shade_hits; g > 0: by pass g - 1);
 * QC_CUR_GEN + g: the work-fetch cursor of pass g. */
#define ACN_MAX_WALK_PASSES 32
enum
{
    QC_TASKS = 0, QC_CLASS0 = 1, QC_CHILDREN = 5, QC_FLAGS = 6, QC_HARD_SHADOW = 7, QC_HARD_PATH = 8,
    QC_CUR_HS = 9, QC_CUR_HP = 10, QC_CUR_HITS = 11, QC_CUR_SHADE0 = 20,   /* .. QC_CUR_SHADE0 + 3: one per size class */
    QS_DEAD_HS = 24,   /* dead slots of the deferred-shadow queue: QC_HARD_SHADOW - QS_HARD_SHADOW - QS_PROBES, counted by k_hard_shadow,
                          which steps over them.  No planner reads it (acn_read_chunk takes the difference) */
    /* ( words 25 .. 27 are unused ) */
    /* reserved slots no record was written to (the unused ends of the waves' reservations): mark - dead = records, exactly.
     * Tasks, path-sample hits, deferred path rays, specular rays (all generations of the level together); the deferred-shadow
     * queue has QS_HARD_SHADOW + QS_PROBES, and QS_DEAD_HS above.  The dead slots of a chunk do not scale with it -- ~64 per wave, queue and launch --
     * so the marks of a SMALL chunk overstate its demand several times (learn_rates) */
    QS_DEAD_T = 28, QS_DEAD_C = 29, QS_DEAD_HP = 30, QS_DEAD_R = 31,
    QS_WALK_RAYS = 12, QS_HARD_SHADOW = 13, QS_HARD_PATH = 14, QS_CHILDREN = 15, QS_TASKS = 16, QS_WALK_STEPS = 17, QS_PRIVATE_RAYS = 18,
    QS_PROBES = 19,   /* specular rays that were answered by an any-hit probe instead of a walk (probe_push) */
    QC_GEN = 32, QC_CUR_GEN = QC_GEN + ACN_MAX_WALK_PASSES + 1,
    QC_N = 104
};

/* slots a wave reserves of a queue per atomic (the queue appends of acn_queues.h) */
#ifndef ACN_QCHUNK
#define ACN_QCHUNK 64
#endif

#endif /* ACN_COUNTS_H */
