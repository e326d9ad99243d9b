// Host code of ignitions during an episode: sf_ignite, sf_ignite_device.
// Part of the single translation unit simfire_hip.hip (included there, behind sf_host_state.h).
#pragma once

// The one scatter launch (enqueue layer): rows (env, column, row, 0) in device memory -> k_ignite, which writes the cell and every
// derived structure the book calls valid - what is not valid is left alone, its rebuild reads the masks.  Behind it, with recording
// on, the arrival pass, as behind every reset - the new sprites are sprites of update commit[e].steps - and a recount of the damage.
static int ignite_rows(sf_sim *s, const int32_t *pts_dev, int n)
{
    IgniteArgs a;
    memset(&a, 0, sizeof a);
    a.g = s->g;
    a.pts = pts_dev; a.n = n;
    a.pl = cur_planes_mut(s); a.age = s->age;
    a.commit = s->commit;
    const bool tiles = s->planes.tiles_kept();
    a.tflags = tiles ? s->tflags : nullptr; a.ring = s->ring;
    a.seam = tiles && s->g.ab == 1 ? s->seam : nullptr;
    a.tdirty = s->planes.hist_all_stale() ? nullptr : s->tdirty;
    a.vbits = s->planes.bits_valid() ? s->vbits : nullptr;
    a.win_hint = s->win_hint;
    SF_TRY(lab_start(s, s->ignite_timer));
    hipLaunchKernelGGL(k_ignite, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, a);
    HIPCHK(hipGetLastError());
    SF_TRY(lab_stop(s, s->ignite_timer));
    s->planes.cells_ignited();
    // The value pass that follows an arrival pass adds the arrivals ABOVE the update its records are summed up to
    // (sf_value_kernels.h), and that update is the one the new cells arrived at: they lie outside its window.  So the arrival pass
    // runs without it (recording off: nothing) and the records are counted again from the plane, which is exact by the invariant of
    // section 20 (no value plane: nothing).
    SF_TRY(arrival_scan(s));
    return value_recount(s);
}

// What both forms check first; *go: there is something to do
static int ignite_begin(sf_sim *s, const char *who, const int32_t *pts, int32_t n, bool *go)
{
    *go = false;
    if (!s) return fail(SF_EINVAL, "%s: null handle", who);
    if (n < 0 || (n > 0 && !pts)) return fail(SF_EINVAL, "%s: bad row list", who);
    *go = n > 0;
    return SF_OK;
}

extern "C" int sf_ignite(sf_sim *s, const int32_t *pts, int32_t n)
{
    bool go;
    SF_TRY(ignite_begin(s, "sf_ignite", pts, n, &go));
    if (!go) return SF_OK;
    const Geo &g = s->g;
    for (int i = 0; i < n; ++i) {
        const int32_t *q = pts + 4 * i;
        if (q[0] < 0 || q[0] >= g.E || q[1] < 0 || q[1] >= g.W || q[2] < 0 || q[2] >= g.H)
            return fail(SF_EINVAL, "sf_ignite: row %d = (env %d, x %d, y %d) is out of range", i, q[0], q[1], q[2]);
        if (q[3] != 0) return fail(SF_EINVAL, "sf_ignite: row %d: reserved = %d must be 0", i, q[3]);
    }
    SF_TRY(begin_call(s, "sf_ignite", kStateCall));
    int slot = 0;
    SF_TRY(pts_stage(s, pts, n, &slot));
    SF_TRY(ignite_rows(s, s->pts_mapped[slot], n));
    HIPCHK(hipEventRecord(s->ev_pts[slot], s->stream));
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_ignite_device(sf_sim *s, const int32_t *device_pts, int32_t n)
{
    bool go;
    SF_TRY(ignite_begin(s, "sf_ignite_device", device_pts, n, &go));
    if (!go) return SF_OK;
    if ((uintptr_t)device_pts & 15) return fail(SF_EINVAL, "sf_ignite_device: the rows must be 16-byte aligned");      // (a lane loads its row whole)
    SF_TRY(begin_call(s, "sf_ignite_device", kStateCall));
    SF_TRY(ignite_rows(s, device_pts, n));
    return finish_call(s, nullptr, !s->async, nullptr);
}

extern "C" int sf_time_ignites(sf_sim *s, int32_t on)
{
    if (!s) return fail(SF_EINVAL, "sf_time_ignites: null handle");
    s->ignite_timer = {on != 0, false};
    return SF_OK;
}

extern "C" int sf_get_ignite_ms(sf_sim *s, float *ms_out)
{
    if (!s || !ms_out) return fail(SF_EINVAL, "sf_get_ignite_ms: null argument");
    return lab_ms(s, s->ignite_timer, "sf_get_ignite_ms", "no ignition has been timed (sf_time_ignites)", ms_out);
}
