// Stand-alone driver of pathtrace_amd/csrc/pt_shape.h, built by hand with -fsanitize=address,undefined (see the header of
// tests/test_launch_shape_cpu.py for the checked properties): walks the sizing over a grid of inputs that crosses its branches
// plus the extremes -- 2^30 pixels, 2^32 - 1 samples, 1 and 304 CUs -- and every launch a plan of the scheduler makes of it.
// Prints "launch_shape_san: N shapes, M launches, 0 failed checks".
#include <cstdio>

#include "../../pathtrace_amd/csrc/pt_shape.h"

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

int main() {
    const uint64_t nps[] = {1, 2, 63, 64, 65, 65521, 1u << 17, (1u << 17) + 1, 1u << 20, 1u << 22, (1u << 22) + 1, 1ull << 26, (1ull << 26) + 1,
                            1ull << 28, 1ull << 30, (1ull << 30) + 1};
    const uint32_t spps[] = {1, 2, 5, 64, 65535, 65536, 3000, 0xFFFFFFFFu};
    const uint64_t caps[] = {0, 8192, 1ull << 40};
    const uint32_t cus[] = {1, 256, 304};
    const uint32_t occs[] = {0, 1, 5, 9};
    unsigned long n_shapes = 0, n_launches = 0;
    for (uint64_t np : nps) for (uint32_t spp : spps) for (uint64_t cap : caps) for (uint32_t n_cus : cus) for (uint32_t occ : occs)
    for (uint32_t variant = 0; variant < 24; ++variant) {
        ptshape::In in{};
        in.np = np; in.spp = spp; in.max_paths_in_flight = cap; in.n_cus = n_cus;
        in.level0_form = variant & 3u;
        in.n_objs = (variant & 4u) ? 129u : 13u; in.blob_f4 = (variant & 4u) ? 0u : 117u;
        in.split_ok = (variant >> 3) & 1u; in.diffuse_only = !in.split_ok;
        in.accel = variant >= 16 && (variant & 1u); in.list = variant >= 16; in.list_regen = variant >= 20; in.inject = variant == 23;
        in.workgroups = variant == 5 ? 100000u : 0u; in.export_below = variant == 6 ? 300u : variant == 7 ? 16u : 0u;
        in.cont_workgroups = variant == 9 ? 100000u : variant == 10 ? 1u : 0u; in.regen_workgroups = variant == 11 ? 7u : 0u;
        in.in_order = variant == 12; in.profile = variant == 13; in.capturing = variant == 14;
        const ptshape::Form f = ptshape::form(in);
        const ptshape::Shape s = ptshape::shape(in, f, occ);
        ++n_shapes;
        CHECK(s.over_cap == (np > s.cap) && s.cap <= ptshape::kMaxPaths);
        if (s.over_cap) continue;
        CHECK(s.nb_max >= 1 && s.n_paths_max <= s.cap && s.grid >= 1 && s.cont_grid >= 1 && s.regen_launch_grid >= 1);
        CHECK(s.n_paths_max <= (uint64_t)s.nw * s.seg_cap);
        CHECK(s.ovf_slots <= (uint64_t)s.nw_cont * s.seg_cap_cont);
        CHECK(!s.regen || s.hand_off);
        if (s.n_batches > 256) continue;              // (a plan has several operations per batch)
        ptsched::State st;
        const ptsched::Plan p = ptsched::plan(st, s.job);
        for (const ptsched::Op& o : p.ops) {
            if (o.kind != ptsched::kOpLaunch) continue;
            const ptshape::Launch l = ptshape::launch(s, o.batch, o.grid, o.level, o.flags);
            ++n_launches;
            CHECK(l.nb >= 1 && l.nb <= s.nb_max && (uint64_t)l.s0 + l.nb <= s.spp);
            if (o.level == 0) {
                CHECK(l.n_first <= (uint64_t)s.nw * l.seg_cap && l.seg_cap <= s.seg_cap);
                CHECK(s.regen || (uint64_t)s.nw * l.seg_cap <= s.q_slots);
                CHECK((uint64_t)l.regen_static * 64u <= (uint64_t)l.n_first + 63u);
            } else {
                CHECK(l.n_first == 0 && (uint64_t)s.nw_cont * l.seg_cap <= (o.own_queue ? s.q_slots_cont : s.q_slots));
            }
            CHECK(l.export_below >= 1);
        }
    }
    std::printf("launch_shape_san: %lu shapes, %lu launches, %d failed checks\n", n_shapes, n_launches, failed);
    return failed != 0;
}
