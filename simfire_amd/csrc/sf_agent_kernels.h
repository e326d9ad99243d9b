// Agents on the device (sf_agents_*): K agents per environment that move on the grid and draw control lines
// where they stand, stepped from a device action tensor.  k_agents_act turns the action words into moves and this tick's
// (column, row, type) points in front of the fire update, k_agents_finish turns the result rows on either side of the update into
// reward (with the tick's loss of value where a value plane is set), done and episode statistics behind it and sends the agents of finished environments back to their start cells.
// Part of simfire_hip.hip only (the run units do not include it).  Both kernels read whichever cell plane is current and convert
// nothing; they write only the agent buffers and the caller's outputs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_common.h"

namespace {

constexpr int kAgentsMax = 64;        // agents per environment: one lane each (the bound of sf_loop_start's points)
// One WAVE per environment: the ballots span the whole workgroup, and k_agents_finish reads done[e] in every lane before lane 0
// overwrites it, which is ordered only inside one wave.
static_assert(kAgentsMax == 64, "the agent kernels are written for workgroups of exactly one wave");

struct AgentArgs {
    Geo g;
    CellPlanes pl;             // the status bytes, in whichever plane is current
    const int32_t *rows;       // the result block [E][8]: running, update() calls, cells per BurnStatus 0..5 - current when the kernel runs
    const int32_t *actions;    // [E][K] action words: move + 5 * interact (k_agents_act)
    int32_t *xyid;             // [E][K][3] (column, row, id): the layout sf_observe takes as agents
    const int32_t *start;      // [E][K][2] where the agents of a finished environment go back to
    int32_t *points;           // [1][E][K][3] this tick's (column, row, type) for sf_step_mitigated; type 0 = padding
    int32_t *prev_cnt;         // [E] BURNING + BURNED cells before the tick
    int32_t *terms;            // [E][4] the reward terms of this tick (act: [1], [3]; finish: [0], [2])
    int32_t *ep_len;           // [E] ticks of the running episode
    double *ep_ret;            // [E] its return
    uint8_t *done;             // [E] act: 1 = the environment was not running before the tick; finish: the tick's done flag (the reset's mask)
    int K, only_unburned, done_on_burn, max_ticks, auto_reset;
    double w[4];               // the reward weights, widened from float
    // values at risk (damage == null: off, and both kernels do what they do without it): damage[e] sits at
    // damage + e * damage_stride bytes and is complete when either kernel runs
    const uint8_t *damage;
    long long damage_stride;
    long long *tick_base;      // [E] act: damage before the tick
    long long *tick_loss;      // [E] finish: damage - tick_base, 0 for an environment that was not running before the tick
    double wv;                 // the fifth weight, widened from float ...
    int wv_on;                 // ... and whether the fifth product is added at all (sf_values_set_weight)
    // the caller's outputs (device memory; any may be null)
    float *o_reward;
    uint8_t *o_done;
    int32_t *o_terms, *o_len;
    double *o_ret;
};

// BurnStatus of cell (x, y) of environment e in the plane that is current (& 7 as k_unpack_status takes it)
__device__ __forceinline__ uint32_t agent_cell(const AgentArgs &a, int e, int x, int y)
{
    return *cell_status(a.pl, a.g, e, y, x) & 7u;
}

// One wave per environment, one lane per agent.  Steps a and b of a tick: the move (one that would leave the grid does not
// happen), the point the agent emits at its NEW cell, the two counts of the wave by ballot, and what k_agents_finish needs from
// before the update.  An environment that is not running keeps its agents and gets padding points.
__global__ __launch_bounds__(kAgentsMax) void k_agents_act(AgentArgs a)
{
    const Geo &g = a.g;
    const int e = blockIdx.x, j = threadIdx.x;
    const int32_t *r0 = a.rows + (long long)e * 8;
    const bool running = r0[0] == 1;
    const bool agent = j < a.K;
    const long long o = ((long long)e * a.K + j) * 3;
    int x = 0, y = 0, type = 0;
    bool blocked = false, emit = false;
    if (agent) { x = a.xyid[o]; y = a.xyid[o + 1]; }
    if (agent && running) {
        int w = a.actions[(long long)e * a.K + j];
        if (w < 0 || w > 19) w = 0;                       // (stay, none)
        const int move = w % 5, interact = w / 5;
        const int nx = x + (move == 4) - (move == 3), ny = y + (move == 2) - (move == 1);
        if (nx < 0 || nx >= g.W || ny < 0 || ny >= g.H) blocked = true;
        else { x = nx; y = ny; }
        if (interact) {
            type = interact + 2;                          // FIRELINE, SCRATCHLINE, WETLINE
            emit = !a.only_unburned || agent_cell(a, e, x, y) == SF_UNBURNED;
        }
        a.xyid[o] = x; a.xyid[o + 1] = y;
    }
    if (agent) { a.points[o] = x; a.points[o + 1] = y; a.points[o + 2] = emit ? type : 0; }
    const int n_emit = __popcll(__ballot(emit)), n_blocked = __popcll(__ballot(blocked));
    if (j == 0) {
        int32_t *t = a.terms + (long long)e * 4;
        t[0] = 0; t[1] = n_emit; t[2] = 0; t[3] = n_blocked;
        a.prev_cnt[e] = r0[3] + r0[4];
        a.done[e] = running ? 0 : 1;
        if (a.damage) a.tick_base[e] = *reinterpret_cast<const long long *>(a.damage + e * a.damage_stride);
    }
}

// The same shape behind the update: steps d and e, and the agent part of f.  The reward is evaluated in double, left to right
// (the translation unit is built with -ffp-contract=off), and rounded to float once; the episode return adds that float.
__global__ __launch_bounds__(kAgentsMax) void k_agents_finish(AgentArgs a)
{
    const int e = blockIdx.x, j = threadIdx.x;
    const int32_t *r1 = a.rows + (long long)e * 8;
    const bool was_off = a.done[e] != 0;                  // (written by k_agents_act; lane 0 overwrites it below, after this load)
    const bool agent = j < a.K;
    const long long o = ((long long)e * a.K + j) * 3;
    bool in_fire = false;
    if (agent && !was_off) in_fire = agent_cell(a, e, a.xyid[o], a.xyid[o + 1]) == SF_BURNING;
    const int n_fire = __popcll(__ballot(in_fire));
    int done = 1;
    if (j == 0) {
        int32_t *t = a.terms + (long long)e * 4;
        int len = a.ep_len[e];
        double ret = a.ep_ret[e];
        float reward = 0.0f;
        long long loss = 0;
        if (a.damage && !was_off) loss = *reinterpret_cast<const long long *>(a.damage + e * a.damage_stride) - a.tick_base[e];
        if (a.damage) a.tick_loss[e] = loss;
        if (was_off) { t[1] = 0; t[3] = 0; }
        else {
            t[0] = (r1[3] + r1[4]) - a.prev_cnt[e];
            t[2] = n_fire;
            double r = a.w[0] * (double)t[0];
            r = r + a.w[1] * (double)t[1];
            r = r + a.w[2] * (double)t[2];
            r = r + a.w[3] * (double)t[3];
            if (a.wv_on) r = r + a.wv * (double)loss;     // (a branch, not "+ 0.0": a sum of -0.0 keeps its sign while the weight is off)
            reward = (float)r;
            len += 1;
            ret = ret + (double)reward;
            done = r1[0] != 1 || (a.done_on_burn && t[2] > 0) || (a.max_ticks > 0 && len >= a.max_ticks);
        }
        if (a.o_reward) a.o_reward[e] = reward;
        if (a.o_done) a.o_done[e] = (uint8_t)done;
        if (a.o_terms) for (int k = 0; k < 4; ++k) a.o_terms[(long long)e * 4 + k] = t[k];
        if (a.o_len) a.o_len[e] = done ? len : 0;
        if (a.o_ret) a.o_ret[e] = done ? ret : 0.0;
        const bool fresh = done && a.auto_reset;          // the environment starts a new episode behind this kernel
        a.ep_len[e] = fresh ? 0 : len;
        a.ep_ret[e] = fresh ? 0.0 : ret;
        a.done[e] = (uint8_t)done;
    }
    done = __shfl(done, 0);
    if (done && a.auto_reset && agent) {
        a.xyid[o] = a.start[((long long)e * a.K + j) * 2];
        a.xyid[o + 1] = a.start[((long long)e * a.K + j) * 2 + 1];
    }
}

// sf_agents_place: entry i puts the K agents of environment envs[i] at xy[i][K][2] (ids j + 1); with also_start these cells become
// the environment's start cells and its episode statistics are cleared.  One thread per (entry, agent).
__global__ void k_agents_place(int n, int K, const int32_t *envs, const int32_t *xy, int also_start, int32_t *xyid, int32_t *start,
                               int32_t *ep_len, double *ep_ret)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * K) return;
    const int e = envs[i / K], j = i % K;
    const long long o = (long long)e * K + j;
    xyid[o * 3] = xy[2 * i]; xyid[o * 3 + 1] = xy[2 * i + 1]; xyid[o * 3 + 2] = j + 1;
    if (also_start) {
        start[o * 2] = xy[2 * i]; start[o * 2 + 1] = xy[2 * i + 1];
        if (j == 0) { ep_len[e] = 0; ep_ret[e] = 0.0; }
    }
}

}  // namespace
