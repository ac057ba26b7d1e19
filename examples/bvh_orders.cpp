// bvh_orders.cpp -- the device-side BVH builds through the C++ mirror: World::new() (the Cornell box), then
// World::scene_rebuild(BvhOrder::Median), scene_rebuild(BvhOrder::Morton) and scene_rebuild(), each followed by bvh_cost().
// Prints one line per build: <order> <cost now> <cost at build> <refits>.
#include <cstdio>

#include "../pathtrace_amd/host/pathtrace.hpp"

using namespace pathtrace;

int main() {
    try {
        World world = World::new_();
        const auto line = [&](const char* name) {
            const World::BvhCost c = world.bvh_cost();
            std::printf("%s %.17g %.17g %u\n", name, c.now, c.at_build, c.refits);
        };
        world.scene_rebuild(World::BvhOrder::Median);
        line("median");
        world.scene_rebuild(World::BvhOrder::Morton);
        line("morton");
        world.scene_rebuild();
        line("default");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
