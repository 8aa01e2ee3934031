// pg_snapshot.h -- device-resident env snapshots: the slot layout of a snapshot store and the argument
// of the copy kernel (pg_snapshot.hip), shared with the host glue (pg_capi.cpp procgen_store_*).
//
// A store is `capacity` slots of `slot_bytes` each in one device allocation.  A slot holds what
// procgen_get_snapshot holds, at fixed 16-byte aligned offsets (the stride is fixed per env handle):
//   0          PGEnv                                   512 B
//   off_ents   PG_NF planes x PG_CAP words             51,200 B  (plane f at f * 2,048 B, as in PGDev::ents)
//   off_mt     rand_gen, level_seed_rand_gen           2 x PG_MT_WORDS words (5,000 B, padded to 5,008)
//   off_grid   int16 cells                             2 B x cells_max
//   off_grid8  the int8 mirror                         1 B x cells_max
//   off_latent the latent row (maze, miner batches)    PG_LATENT_N words (4,924 B, padded to 4,928)
//   off_bg     the generated background                PG_GEN_BG_PX words (use_generated_assets)
// cells_max = the largest pg_game_max_w x pg_game_max_h over the games of the batch, rounded up to 16.
// Only the live part of each region is copied: num_ents slots from the bottom and num_tail from the top
// of every plane, main_width x main_height cells (the mirror only while grid8_ok), and the two
// generators, the latent row and the background whole.
#pragma once
#include "pg_engine.h"

struct PGSnapLayout {
    uint32_t off_ents, off_mt, off_grid, off_grid8, off_latent, off_bg; // off_latent / off_bg: 0 = not carried
    uint32_t cells_max;
    uint64_t slot_bytes;
};

static inline PGSnapLayout pg_snap_layout(const int *games, int num_games, bool latent, bool gen_bg) {
    auto up16 = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
    PGSnapLayout l{};
    uint32_t cells = 0;
    for (int k = 0; k < num_games; k++) {
        const uint32_t c = (uint32_t)(pg_game_max_w(games[k]) * pg_game_max_h(games[k]));
        if (c > cells) cells = c;
    }
    if (cells > PG_GRID_MAX) cells = PG_GRID_MAX;
    l.cells_max = (uint32_t)up16(cells);
    uint64_t o = sizeof(PGEnv);
    l.off_ents = (uint32_t)o; o += (uint64_t)PG_ENT_BLOCK * 4;
    l.off_mt = (uint32_t)o; o = up16(o + 2 * PG_MT_WORDS * 4);
    l.off_grid = (uint32_t)o; o += (uint64_t)l.cells_max * 2;
    l.off_grid8 = (uint32_t)o; o += l.cells_max;
    if (latent) { l.off_latent = (uint32_t)o; o = up16(o + (uint64_t)PG_LATENT_N * 4); }
    if (gen_bg) { l.off_bg = (uint32_t)o; o += (uint64_t)PG_GEN_BG_PX * 4; }
    l.slot_bytes = o;
    return l;
}

// The copy kernel's argument: the env arrays it moves (a subset of PGDev's pointers), the store and the
// (env, slot) pairs.  to_env = 0: env_ids[k] -> slots[k] (save); 1: slots[k] -> env_ids[k] (load), which
// also writes the env's five output scalars from the state's step data and drops its prefetched spare.
struct PGSnap {
    PGEnv *envs;
    float *ents;
    int16_t *grid;
    int8_t *grid8;
    uint32_t *mt;
    int32_t *latent;  // null: no latent rows
    uint32_t *gen_bg; // null: atlas backgrounds
    float *rew;
    uint8_t *first;
    int32_t *prev_level_seed;
    uint8_t *prev_level_complete;
    int32_t *level_seed;
    int32_t *sp_gen;  // null: no level prefetch
    uint8_t *store;
    PGSnapLayout lay;
    const int32_t *env_ids;
    const int32_t *slots;
    int32_t count;
};

extern "C" void pg_launch_snapshot(const PGSnap *a, int to_env, hipStream_t s);
