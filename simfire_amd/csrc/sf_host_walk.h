// Host code of sf_walk: walking distance to target cells through walkable cells.  Included once from
// simfire_hip.hip, behind sf_host_views.h (whose sf_reach it follows word for word in what a call may and may not do).
#pragma once

// The environment list goes through the feature's call block; the list is then worked through in chunks of as many environments as
// the scratch budget holds (walk_env_bytes each), one k_walk launch per chunk with one workgroup per listed environment.  All of it
// on the handle's stream; no state of the handle changes but the scratch.
extern "C" int sf_walk(sf_sim *s, const sf_walk_params *p, int32_t n, const int32_t *envs, const sf_walk_out *out)
{
    if (!s || !p || !out) return fail(SF_EINVAL, "sf_walk: null argument");
    const Geo &g = s->g;
    if (n < 0 || (n > 0 && !envs)) return fail(SF_EINVAL, "sf_walk: bad environment list");
    if (p->target_mask < 0 || p->target_mask > 63) return fail(SF_EINVAL, "sf_walk: target_mask %d (bit s selects BurnStatus s: 0..63)", p->target_mask);
    if (p->through_mask < 1 || p->through_mask > 63) return fail(SF_EINVAL, "sf_walk: through_mask %d (bit s selects BurnStatus s: 1..63)", p->through_mask);
    if (p->target_mask == 0 && !p->targets) return fail(SF_EINVAL, "sf_walk: target_mask 0 needs a targets plane");
    if (p->connectivity != 0 && p->connectivity != 4 && p->connectivity != 8)
        return fail(SF_EINVAL, "sf_walk: connectivity %d (0 or 4: the agents' moves, 8)", p->connectivity);
    if (p->k < 0 || p->k > SF_DIST_MAX_POINTS) return fail(SF_EINVAL, "sf_walk: %d points per environment (0..%d)", p->k, SF_DIST_MAX_POINTS);
    if (p->k > 0 && !p->points) return fail(SF_EINVAL, "sf_walk: k = %d needs points", p->k);
    if (p->k == 0 && p->points) return fail(SF_EINVAL, "sf_walk: points need k > 0");
    if ((out->point_moves || out->point_step) && p->k == 0) return fail(SF_EINVAL, "sf_walk: point_moves and point_step need k > 0");
    if (out->point_step && p->connectivity == 8) return fail(SF_EINVAL, "sf_walk: point_step needs connectivity 4 (the four moves)");
    if (p->max_moves < 0) return fail(SF_EINVAL, "sf_walk: max_moves %d (0: no cap)", p->max_moves);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(SF_EINVAL, "sf_walk: reserved must be 0");
    if (!out->moves && !out->point_moves && !out->point_step && !out->reached && !out->levels)
        return fail(SF_EINVAL, "sf_walk: every output is null");
    if (((uintptr_t)out->moves | (uintptr_t)out->point_moves | (uintptr_t)out->point_step | (uintptr_t)out->reached | (uintptr_t)out->levels) & 3)
        return fail(SF_EINVAL, "sf_walk: an output is not aligned to its element");
    const size_t need = (size_t)walk_env_bytes(g);
    if (p->scratch_bytes < 0 || (p->scratch_bytes > 0 && (size_t)p->scratch_bytes < need))
        return fail(SF_EINVAL, "sf_walk: scratch_bytes %lld is less than one environment's need (%zu bytes)", (long long)p->scratch_bytes, need);
    SF_TRY(check_envs(s, "sf_walk", n, envs));
    if (g.W > kWalkMaxWidth) return fail(SF_ENOTSUP, "sf_walk: grids wider than %d cells are not supported (width %d)", kWalkMaxWidth, g.W);
    SF_TRY(check_ready(s, "sf_walk", kNeedRt | kNeedReset));
    SF_TRY(begin_call(s, "sf_walk", kNeedRt | kNeedReset | kNotVoid));
    if (n == 0) return SF_OK;

    const size_t budget = p->scratch_bytes > 0 ? (size_t)p->scratch_bytes : (size_t)kWalkScratchDefault;
    const int chunk = (int)std::min<size_t>({(size_t)n, std::max<size_t>(budget / need, 1), (size_t)65535});
    WalkState &w = s->walk;
    if ((size_t)chunk * need > w.cap) {               // growing waits for the device: enqueued kernels may still use the scratch
        HIPCHK(hipStreamSynchronize(s->stream));
        s->bytes -= (int64_t)w.cap;
        HIPCHK(w.release());
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&w.mem), (size_t)chunk * need));
        w.cap = (size_t)chunk * need;
        s->bytes += (int64_t)w.cap;
    }
    // the call block: the environment list | one WalkArgs per chunk (the kernel takes its arguments from there)
    const int chunks = (n + chunk - 1) / chunk;
    const size_t o_args = ((size_t)n * sizeof(int32_t) + 15) / 16 * 16, bytes = o_args + (size_t)chunks * sizeof(WalkArgs);
    SF_TRY(block_reserve(s, w.blk, bytes));
    memcpy(w.blk.pinned, envs, (size_t)n * sizeof(int32_t));

    WalkArgs a;
    memset(&a, 0, sizeof a);
    ReachArgs &r = a.r;
    r.g = g;
    r.status = s->status;
    r.cells = s->bl_cur ? s->cells : nullptr;
    r.passable = p->passable;
    r.pass_env = p->passable_per_env ? (long long)g.H * g.W : 0;
    r.pass_vec = p->passable && g.W % 16 == 0 && !((uintptr_t)p->passable & 15);
    a.targets = p->targets;
    a.tgt_env = p->targets_per_env ? (long long)g.H * g.W : 0;
    a.tgt_vec = p->targets && g.W % 16 == 0 && !((uintptr_t)p->targets & 15);
    r.k = p->k;
    r.scratch = w.mem;
    r.scratch_env = (long long)need;
    for (int st = 0; st < 6; ++st) {
        if ((p->target_mask >> st) & 1) (st < 4 ? r.slo : r.shi) |= 1u << (8 * (st & 3));
        if ((p->through_mask >> st) & 1) (st < 4 ? r.tlo : r.thi) |= 1u << (8 * (st & 3));
    }
    r.conn8 = p->connectivity == 8;
    a.max_moves = p->max_moves;
    r.WORDS = reach_words(g); r.BR = reach_band_rows(g); r.nb = r.BR * r.WORDS;
    a.moves_vec = out->moves && g.W % 4 == 0 && !((uintptr_t)out->moves & 15);
    for (int c = 0; c < chunks; ++c) {
        const int c0 = c * chunk;
        r.envs = reinterpret_cast<const int32_t *>(w.blk.dev) + c0;
        r.points = p->k ? p->points + (size_t)c0 * p->k * 3 : nullptr;
        a.moves = out->moves ? out->moves + (size_t)c0 * g.H * g.W : nullptr;
        a.point_moves = out->point_moves ? out->point_moves + (size_t)c0 * p->k : nullptr;
        a.point_step = out->point_step ? out->point_step + (size_t)c0 * p->k : nullptr;
        a.reached = out->reached ? out->reached + c0 : nullptr;
        a.levels = out->levels ? out->levels + c0 : nullptr;
        memcpy(w.blk.pinned + o_args + (size_t)c * sizeof(WalkArgs), &a, sizeof a);
    }
    SF_TRY(block_send(s, w.blk, bytes));

    // one band per thread: the front stays in registers and U in LDS for the whole search (k_walk<true>: 156 KiB at 1024 threads); else
    // passes of 1024 bands over the scratch planes.  Every point has a lane of its own, so a small grid still gets k threads.
    const bool resident = r.nb <= kWalkThreads;
    const unsigned threads = resident ? (unsigned)((std::max(r.nb, p->k) + 63) / 64 * 64) : (unsigned)kWalkThreads;
    const size_t lds = walk_lds_bytes((int)threads, resident);
    const void *fn = resident ? reinterpret_cast<const void *>(&k_walk<true>) : reinterpret_cast<const void *>(&k_walk<false>);
    HIPCHK(allow_lds(s, fn, lds));
    for (int c = 0; c < chunks; ++c) {
        const WalkArgs *ap = reinterpret_cast<const WalkArgs *>(w.blk.dev + o_args) + c;
        const unsigned cn = (unsigned)std::min(chunk, n - c * chunk);
        if (resident) hipLaunchKernelGGL(k_walk<true>, dim3(cn), dim3(threads), lds, s->stream, ap);
        else hipLaunchKernelGGL(k_walk<false>, dim3(cn), dim3(threads), lds, s->stream, ap);
    }
    return finish_call(s, "sf_walk", !s->async, nullptr);
}
