// pt_sched.cpp -- pt_debug_sched_*: the launch planner of pt_sched.h on a scheduling state of its own (host only, no HIP);
// pt_debug_render_shape: the launch sizing of pt_shape.h on the caller's numbers.
// What pt_api.cpp's render_impl does with a context's state -- plan on a copy, execute, commit; recover on a failure -- is
// done here with the "execute" step left to the caller: tests/test_sched_cpu.py simulates the streams.
#include <cstring>
#include <new>

#include "../../include/pathtrace_amd.h"
#include "pt_sched.h"
// tests/test_sched_mutants_cpu.py builds this file with nothing but a mutant of pt_sched.h beside it: the planner's entries alone
#if __has_include("pt_shape.h")
#include "pt_shape.h"
#define PT_HAVE_SHAPE 1
#endif

// pt_host.cpp; declared here and not through pt_context.h: this file also builds on its own with a plain host compiler and no
// HIP headers (tests/test_sched_mutants_cpu.py)
int pt_internal_fail(int code, const char* fmt, ...);

struct PtSched {
    ptsched::State state;
};

static_assert(sizeof(PtSchedOp) == sizeof(ptsched::Op), "PtSchedOp mirrors ptsched::Op");
static_assert(sizeof(PtSchedJob) == 14 * sizeof(uint32_t) + sizeof(uint64_t), "PtSchedJob layout");
#ifdef PT_HAVE_SHAPE
static_assert(sizeof(PtShapeIn) == sizeof(ptshape::In) && sizeof(PtShapeIn) == 2 * sizeof(uint64_t) + 20 * sizeof(uint32_t), "PtShapeIn mirrors ptshape::In");
static_assert(sizeof(PtShapeLaunch) == sizeof(ptshape::Launch) + sizeof(uint32_t), "PtShapeLaunch mirrors ptshape::Launch (+ 1 reserved word)");
#endif

extern "C" {

int pt_debug_sched_create(PtSched** out) {
    if (!out) return pt_internal_fail(PT_ERR_INVALID_ARG, "pt_debug_sched_create: out is null");
    *out = new (std::nothrow) PtSched();
    return *out ? PT_OK : pt_internal_fail(PT_ERR_OOM, "pt_debug_sched_create: out of memory");
}

void pt_debug_sched_destroy(PtSched* s) { delete s; }

int pt_debug_sched_render(PtSched* s, const PtSchedJob* job, uint32_t faults, uint32_t fail_after, PtSchedOp* ops, uint32_t cap,
                          uint32_t* n_ops, uint32_t* lanes) {
    if (!s || !job || !n_ops || (!ops && cap)) return pt_internal_fail(PT_ERR_INVALID_ARG, "pt_debug_sched_render: null argument");
    ptsched::Job j;
    j.n_batches = job->n_batches; j.regen = job->regen; j.split = job->regen ? job->split : 0u; j.hand_off = job->hand_off;
    j.regen_export = job->regen_export; j.profile = job->profile; j.in_order = job->in_order; j.capturing = job->capturing;
    j.grid = job->grid; j.regen_grid = job->regen_grid; j.cont_grid = job->cont_grid; j.regen_capacity = job->regen_capacity;
    j.fixed_grid = job->fixed_grid; j.counter_words = job->counter_words; j.xchg_need = j.split ? job->xchg_need : 0u;
    if (j.regen && !j.hand_off) return pt_internal_fail(PT_ERR_INVALID_ARG, "pt_debug_sched_render: a regenerating launch uses the chunk counters (hand_off = 1)");
    ptsched::State next = s->state;                        // render_impl: plan on a copy ...
    ptsched::Plan p = ptsched::plan(next, j, faults);
    if (lanes) *lanes = p.lanes ? 1u : 0u;
    size_t n = p.ops.size();
    const bool failed = fail_after < n;
    if (failed) {
        // ... the operations before the failing one were enqueued; the recovery waits for every stream and starts the state over
        n = fail_after;
        ptsched::Op sync{};
        sync.kind = ptsched::kOpHostSync;
        p.ops.resize(n);
        p.ops.push_back(sync);
        n += 1;
        ptsched::on_failure(s->state, next);
    } else {
        s->state = next;                                    // ... and commit it after the last operation
    }
    *n_ops = (uint32_t)n;
    if (n > cap) return pt_internal_fail(PT_ERR_INVALID_ARG, "pt_debug_sched_render: %zu operations, room for %u", n, cap);
    if (n) std::memcpy(ops, p.ops.data(), n * sizeof(PtSchedOp));
    return failed ? PT_ERR_HIP : PT_OK;
}

#ifdef PT_HAVE_SHAPE
int pt_debug_render_shape(const PtShapeIn* in, uint32_t occupancy, PtShapeOut* out, const PtSchedOp* ops, uint32_t n_ops, PtShapeLaunch* launches) {
    if (!in || !out || (n_ops && (!ops || !launches))) return pt_internal_fail(PT_ERR_INVALID_ARG, "pt_debug_render_shape: null argument");
    if (in->np == 0 || in->spp == 0 || in->n_cus == 0) return pt_internal_fail(PT_ERR_INVALID_ARG, "pt_debug_render_shape: np, spp and n_cus must be > 0");
    ptshape::In i;
    std::memcpy(&i, in, sizeof i);
    const ptshape::Form f = ptshape::form(i);
    const ptshape::Shape s = ptshape::shape(i, f, occupancy);
    std::memset(out, 0, sizeof *out);
    out->lds_job = f.lds_job; out->split = f.split; out->regen_scene = f.regen_scene; out->over_cap = s.over_cap;
    out->cap = s.cap;
    if (s.over_cap) return PT_ERR_UNSUPPORTED;             // as render_impl answers; `out` says why
    out->n_paths_max = s.n_paths_max; out->ovf_slots = s.ovf_slots; out->q_slots_cont = s.q_slots_cont; out->q_slots = s.q_slots;
    out->np = s.np; out->spp = s.spp; out->nb_max = s.nb_max; out->n_batches = s.n_batches;
    out->export_small = s.export_small; out->paths_per_wave = s.paths_per_wave; out->small_scene = s.small_scene;
    out->hand_off = s.hand_off; out->regen = s.regen; out->overlap = s.overlap;
    out->grid = s.grid; out->nw = s.nw; out->seg_cap = s.seg_cap;
    out->regen_per_cu = s.regen_per_cu; out->regen_capacity = s.regen_capacity; out->regen_grid = s.regen_grid;
    out->regen_launch_grid = s.regen_launch_grid; out->cont_grid = s.cont_grid; out->nw_cont = s.nw_cont;
    out->seg_cap_cont = s.seg_cap_cont; out->regen_export = s.regen_export;
    const ptsched::Job& j = s.job;
    PtSchedJob& o = out->job;
    o.n_batches = j.n_batches; o.regen = j.regen; o.split = j.split; o.hand_off = j.hand_off; o.regen_export = j.regen_export;
    o.profile = j.profile; o.in_order = j.in_order; o.capturing = j.capturing; o.grid = j.grid; o.regen_grid = j.regen_grid;
    o.cont_grid = j.cont_grid; o.regen_capacity = j.regen_capacity; o.fixed_grid = j.fixed_grid; o.counter_words = j.counter_words;
    o.xchg_need = j.xchg_need;
    for (uint32_t k = 0; k < n_ops; ++k) {
        std::memset(&launches[k], 0, sizeof launches[k]);
        if (ops[k].kind != ptsched::kOpLaunch) continue;
        if (ops[k].batch >= s.n_batches || ops[k].grid == 0)
            return pt_internal_fail(PT_ERR_INVALID_ARG, "pt_debug_render_shape: operation %u is not a launch of this render", k);
        const ptshape::Launch l = ptshape::launch(s, ops[k].batch, ops[k].grid, ops[k].level, ops[k].flags);
        std::memcpy(&launches[k], &l, sizeof l);
    }
    return PT_OK;
}
#endif

int pt_debug_sched_sync(PtSched* s, uint32_t collect) {
    if (!s) return pt_internal_fail(PT_ERR_INVALID_ARG, "pt_debug_sched_sync: null argument");
    const bool c = collect != 0 && s->state.stats_pending != 0;
    ptsched::on_sync(s->state, c, true);
    return PT_OK;
}

}  // extern "C"
