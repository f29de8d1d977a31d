// emu_score.cpp -- the score kernel's phase bodies (copra_amd/csrc/score_step.hpp) on the host: a walker over the four phases with a NaN-filled
// image, the guard words and the walk orders of emu_walk.h, and the summary's reduction with its documented tree applied lane by lane.
// Compile with -ffp-contract=off: the expectation (tests/score_ref.py) rounds every product and every sum.
#include "emu_score.h"

#include "../../copra_amd/csrc/score_step.hpp"
#include "emu_walk.h"

#include <vector>

using namespace copra_hip;

// one workgroup of the reduce kernel: every thread's fold, the lane tree of every wave, the fold of the waves
template <class Part, class Fold, class Merge>
static Part reduce_part(Fold fold, Merge merge)
{
    std::vector<Part> lane((size_t)kScoreThreads);
    for (int tid = 0; tid < kScoreThreads; ++tid) lane[(size_t)tid] = fold(tid);
    for (int w = 0; w < kScoreThreads / 64; ++w)
        for (int off = 32; off >= 1; off >>= 1)
            for (int l = 0; l + off < 64; ++l) // (ascending: lane l + off still holds the value of before this step)
                lane[(size_t)(64 * w + l)] = merge(lane[(size_t)(64 * w + l)], lane[(size_t)(64 * w + l + off)]);
    Part acc = lane[0];
    for (int w = 1; w < kScoreThreads / 64; ++w) acc = merge(acc, lane[(size_t)(64 * w)]);
    return acc;
}
static ScoreSummary reduce_workgroup(const ScoreReduceArgs& R, int wg)
{
    ScoreSummary out;
    for (int f = 0; f < kScoreFields; ++f)
        out.f[f] = reduce_part<ScoreStat>([&](int tid) { return score_fold_stat(R, wg, tid, f); }, [](const ScoreStat& a, const ScoreStat& b) { return score_stat_merge(a, b); });
    out.c = reduce_part<ScoreCounts>([&](int tid) { return score_fold_counts(R, wg, tid); }, [](const ScoreCounts& a, const ScoreCounts& b) { return score_counts_merge(a, b); });
    return out;
}

extern "C" {

int emu_score_tick(EmuScoreTick* t)
{
    ScoreArgs S {};
    S.batch = t->batch, S.nx = t->nx, S.nu = t->nu, S.group = t->group;
    S.dense = t->dense, S.per_instance = t->per_instance;
    S.x = t->x, S.u = t->u, S.age = t->age;
    S.qx = t->qx, S.ru = t->ru, S.x_ref = t->x_ref;
    S.ref_steps = t->x_ref ? t->ref_steps : 1;
    const long long tau = t->tau < 0 ? 0 : t->tau;
    S.ref_row = tau < S.ref_steps - 1 ? tau : S.ref_steps - 1;
    S.x_lo = t->x_lo, S.x_hi = t->x_hi, S.u_lo = t->u_lo, S.u_hi = t->u_hi;
    S.tol = t->tol;
    S.rec = static_cast<ScoreRecord*>(t->rec);
    S.vec2 = t->vec2_mode < 0 ? score_vec2_ok(S) : 0;
    t->vec2_used = S.vec2;
    const ScoreLds L = score_lds(S);
    t->lds_doubles = L.total;
    emu::Image img((size_t)L.total);
    if (!img.lds) return emu::kEmuNoMemory;
    const int grid = (S.batch + S.group - 1) / S.group;
    return emu::walk(img, grid, 4, t->threads, t->order, t->seed, [&](int wg, int ph, int tid) {
        if (ph == 0) score_stage(S, wg, tid, t->threads, img.lds);
        else if (ph == 1) score_rows(S, wg, tid, t->threads, img.lds);
        else if (ph == 2) score_fold(S, wg, tid, t->threads, img.lds);
        else score_store(S, wg, tid, t->threads, img.lds);
    });
}

int emu_score_reduce(long long count, const void* rec, void* out)
{
    ScoreSummary res = score_empty();
    if (count > 0) {
        const long long chunks = score_chunks(count);
        std::vector<ScoreSummary> part((size_t)chunks);
        ScoreReduceArgs R {};
        R.stage = 1, R.count = count, R.rec = static_cast<const ScoreRecord*>(rec);
        for (long long c = 0; c < chunks; ++c) part[(size_t)c] = reduce_workgroup(R, (int)c);
        R.stage = 2, R.count = chunks, R.rec = nullptr, R.partials = part.data();
        res = reduce_workgroup(R, 0);
    }
    std::memcpy(out, &res, sizeof res);
    return 0;
}

long long emu_score_image_bytes(int nx, int nu, int dense) { return (long long)score_image_bytes(nx, nu, dense); }
int emu_score_launch_group(int nx, int nu, int dense) { return score_group(nx, nu, dense); }
int emu_score_layout(int nx, int nu, int group, const int* f, int* out)
{
    const ScoreLds L = score_lds(nx, nu, group, f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]);
    const int v[14] = { L.ox, L.ou, L.oag, L.orec, L.oqx, L.oru, L.oref, L.oxl, L.oxh, L.oul, L.ouh, L.oc, L.ov, L.total };
    for (int i = 0; i < 14; ++i) out[i] = v[i];
    return 14;
}
int emu_score_chunk(void) { return kScoreChunk; }
int emu_score_threads(void) { return kScoreThreads; }
int emu_score_sizes(int* record, int* stat, int* summary)
{
    *record = (int)sizeof(ScoreRecord), *stat = (int)sizeof(ScoreStat), *summary = (int)sizeof(ScoreSummary);
    return 0;
}
}
