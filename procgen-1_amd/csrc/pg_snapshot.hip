// pg_snapshot.hip -- device-resident env snapshots: one kernel moves env states between the engine's
// per-env arrays and the slots of a snapshot store (pg_snapshot.h), in either direction.
//
// One wavefront per (env, slot) pair, grid stride over the pairs.  The wave reads the PGEnv first (one
// 8-byte load per lane) and takes the live sizes from it, then copies only the live data with 16-byte
// accesses: the entity planes as one flattened range of (plane, slot quad) items so every lane stays busy
// whatever num_ents is, the grid cells, the int8 mirror while it is current, the two generators (8-byte
// accesses: an env's generators start at a multiple of 5,000 B), the latent row (4-byte accesses: rows
// of 4,924 B) and the generated background.  Four loads are in flight per lane before the first store.
// Nothing on the device can fail: the pairs are checked on the host and the states come from the engine.
#include "pg_snapshot.h"

namespace {

#define SNAP_LANE ((int)threadIdx.x)

// dst[idx(k)] = src[idx(k)] for k < total, lanes along k
template <typename T, typename IDX>
__device__ __forceinline__ void snap_copy(const T *__restrict__ src, T *__restrict__ dst, int total, IDX idx) {
    int k = SNAP_LANE;
    for (; k + 192 < total; k += 256) { // four loads in flight per lane before the first store
        const int i0 = idx(k), i1 = idx(k + 64), i2 = idx(k + 128), i3 = idx(k + 192);
        const T r0 = src[i0], r1 = src[i1], r2 = src[i2], r3 = src[i3];
        dst[i0] = r0;
        dst[i1] = r1;
        dst[i2] = r2;
        dst[i3] = r3;
    }
    for (; k < total; k += 64) {
        const int i = idx(k);
        dst[i] = src[i];
    }
}

template <typename T>
__device__ __forceinline__ void snap_copy(const void *src, void *dst, int total) {
    snap_copy(reinterpret_cast<const T *>(src), reinterpret_cast<T *>(dst), total, [](int k) { return k; });
}

// word i of the PGEnv the wave holds as one uint2 per lane
#define SNAP_WORD(member) \
    ((int32_t)__builtin_amdgcn_readlane(((offsetof(PGEnv, member) / 4) & 1) ? w.y : w.x, (int)(offsetof(PGEnv, member) / 8)))

template <bool TO_ENV>
__global__ __launch_bounds__(64) void pg_snapshot_kernel(PGSnap a) {
    const PGSnapLayout &l = a.lay;
    for (int p = (int)blockIdx.x; p < a.count; p += (int)gridDim.x) {
        const int env = a.env_ids[p];
        uint8_t *const sb = a.store + (size_t)a.slots[p] * l.slot_bytes;
        // src / dst of one region: the env's array or the slot's block
#define SNAP_SRC(envp, off) (TO_ENV ? (const void *)(sb + (off)) : (const void *)(envp))
#define SNAP_DST(envp, off) (TO_ENV ? (void *)(envp) : (void *)(sb + (off)))
        const uint2 w = reinterpret_cast<const uint2 *>(SNAP_SRC(a.envs + env, 0))[SNAP_LANE];
        const int game = SNAP_WORD(game_id);
        const int ne = min(max(SNAP_WORD(num_ents), 0), PG_CAP);
        const int nt = min(max(SNAP_WORD(num_tail), 0), PG_CAP - ne);
        const int cells = min(max(SNAP_WORD(main_width) * SNAP_WORD(main_height), 0), (int)l.cells_max);

        // entity planes: plane f = uint4 [f * 128, (f + 1) * 128); the live slots are the quads
        // [0, q) from the bottom and [t0, 128) from the top (a quad both ranges cover is copied twice)
        float *const eb = a.ents + (size_t)env * PG_ENT_BLOCK;
        const uint4 *es = reinterpret_cast<const uint4 *>(SNAP_SRC(eb, l.off_ents));
        uint4 *ed = reinterpret_cast<uint4 *>(SNAP_DST(eb, l.off_ents));
        const int q = (ne + 3) >> 2;
        if (q > 0) snap_copy(es, ed, PG_NF * q, [q](int k) { const int f = k / q; return f * (PG_CAP / 4) + (k - f * q); });
        if (nt > 0) {
            const int t0 = (PG_CAP - nt) >> 2, qt = PG_CAP / 4 - t0;
            snap_copy(es, ed, PG_NF * qt, [qt, t0](int k) { const int f = k / qt; return f * (PG_CAP / 4) + t0 + (k - f * qt); });
        }
        int16_t *const gb = a.grid + (size_t)env * PG_GRID_MAX;
        snap_copy<uint4>(SNAP_SRC(gb, l.off_grid), SNAP_DST(gb, l.off_grid), (cells + 7) >> 3);
        if (SNAP_WORD(grid8_ok)) { // the mirror travels with its flag
            int8_t *const g8 = a.grid8 + (size_t)env * PG_GRID_MAX;
            snap_copy<uint4>(SNAP_SRC(g8, l.off_grid8), SNAP_DST(g8, l.off_grid8), (cells + 15) >> 4);
        }
        uint32_t *const mb = a.mt + (size_t)env * 2 * PG_MT_WORDS;
        snap_copy<uint2>(SNAP_SRC(mb, l.off_mt), SNAP_DST(mb, l.off_mt), PG_MT_WORDS);
        if (a.latent && (game == PG_GAME_MAZE || game == PG_GAME_MINER)) {
            int32_t *const lb = a.latent + (size_t)env * PG_LATENT_N;
            snap_copy<uint32_t>(SNAP_SRC(lb, l.off_latent), SNAP_DST(lb, l.off_latent), PG_LATENT_N);
        }
        if (a.gen_bg) {
            uint32_t *const bb = a.gen_bg + (size_t)env * PG_GEN_BG_PX;
            snap_copy<uint4>(SNAP_SRC(bb, l.off_bg), SNAP_DST(bb, l.off_bg), PG_GEN_BG_PX / 4);
        }
        reinterpret_cast<uint2 *>(SNAP_DST(a.envs + env, 0))[SNAP_LANE] = w;
        if (TO_ENV && SNAP_LANE == 0) {
            // what Game::observe reports of a restored state (game.cpp:173-191), as procgen_set_snapshot
            a.rew[env] = __int_as_float(SNAP_WORD(sd_reward));
            a.first[env] = (uint8_t)(SNAP_WORD(sd_done) != 0);
            a.prev_level_seed[env] = SNAP_WORD(prev_level_seed);
            a.prev_level_complete[env] = (uint8_t)(SNAP_WORD(sd_level_complete) != 0);
            a.level_seed[env] = SNAP_WORD(current_level_seed);
            if (a.sp_gen) a.sp_gen[env] = PG_SP_NONE; // its spare was made from another level-seed generator
        }
#undef SNAP_SRC
#undef SNAP_DST
    }
}

static_assert(PG_CAP % 4 == 0 && PG_GRID_MAX % 16 == 0 && PG_GEN_BG_PX % 4 == 0 && sizeof(PGEnv) == 64 * 8,
              "the 16-byte copies rely on these");

} // namespace

extern "C" void pg_launch_snapshot(const PGSnap *a, int to_env, hipStream_t s) {
    if (a->count <= 0) return;
    // 8,192 waves fill the 256 CUs (32 waves each); more pairs than that share them by the grid stride
    const int g = a->count < 8192 ? a->count : 8192;
    if (to_env) hipLaunchKernelGGL(pg_snapshot_kernel<true>, dim3(g), dim3(64), 0, s, *a);
    else hipLaunchKernelGGL(pg_snapshot_kernel<false>, dim3(g), dim3(64), 0, s, *a);
}
