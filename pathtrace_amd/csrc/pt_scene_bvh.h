// pt_scene_bvh.h -- the device BVH of a context's scene as one object: struct DeviceBvh (PtContext::tree), and the output contract
// of a tree export (struct BvhExport).  pt_context.h includes this file behind the owners it is made of; pt_scene_bvh.cpp.
//
// The tree has three lives: built on the host at first use and uploaded (adopt), refitted on the device to a new pose
// of the same objects (enqueue_refit, 5e), built on the device in Morton or median order (enqueue_build + enqueue_refit, 5f / 5i).
// Its invariants, each kept by the operations below and by nothing else:
//   I1  has <=> view.bvh names the four arrays and the root of a tree over the uploaded scene's n_nodes nodes and n_slots leaf
//       slots, and `order` / height_first hold that tree's nodes by height (one refit launch per height).  !has: view.bvh is empty.
//   I2  refused / failed (only while !has): the scene has a NaN/inf coordinate / the host builder's tree is deeper than the
//       traversal stack -- properties of the scene: no render builds again, PT_ACCEL_AUTO stays with the linear scan (may_build).
//   I3  topo.n = the object count whose ptbvh::morton_topology topo.* hold (codes and order on the device, the rest here), med_n
//       likewise for ptbvh::median_plan; -1: none, and -1 WHILE their device arrays are being rewritten, so a copy that fails
//       midway leaves "none".  Both are planned once per object count.
//   I4  is_morton: the code words of `nodes` and `order` hold topo's (a device build then skips rewriting them).  The host builder
//       writes another topology; growing `nodes` or `order` drops their content: both clear the flag.
//   I5  growing any array of the tree drops the tree (DevBuf::ensure frees first): a reservation that fails midway leaves !has.
//   I6  cost_on_device says which record holds the cost of the tree as built: cost_build (host builder, in the grid it built
//       with), or the sums in cost_built counted in the grid cell cost_cell (device build; copied on the stream behind the last
//       level launch).  cost_sums are the sums of the tree as it stands; refits counts the refits since the build.
#pragma once
#include "pt_bvh.h"

// What the tree exports write (pt_debug_bvh_refit_check / _morton_check / _median_check, pt_debug_bvh_read): up to cap_nodes nodes
// of 16 words, up to cap_slots leaf slots (12 + 4 floats and an id each), grid[7] = min, cell, scene_abs; every pointer optional.
struct BvhExport {
    uint32_t* qnodes; uint32_t cap_nodes;
    float *leaf_rec, *leaf_lead; uint32_t* leaf_ids; uint32_t cap_slots;
    float* grid; uint32_t* root; uint64_t* cost_now;
    bool null_array() const { return (cap_nodes && !qnodes) || (cap_slots && (!leaf_rec || !leaf_lead || !leaf_ids)); }
    size_t nodes(size_t have) const { return have < cap_nodes ? have : cap_nodes; }
    size_t slots(size_t have) const { return have < cap_slots ? have : cap_slots; }
    void scalars(const float grid_min[3], const float grid_cell[3], float scene_abs, uint32_t root_code) const {
        if (grid) {
            for (int k = 0; k < 3; ++k) { grid[k] = grid_min[k]; grid[3 + k] = grid_cell[k]; }
            grid[6] = scene_abs;
        }
        if (root) *root = root_code;
    }
};

struct DeviceBvh {
    // What a device build of n objects needs from the host, planned before anything is touched (plan): the topology and the
    // median plan where the cached ones are another count's (I3), and the tree's size either way.
    struct Rebuild {
        uint32_t n = 0, nodes = 0, slots = 0;
        bool median = false, new_topo = false, new_plan = false;
        ptbvh::Topology topo;
        ptbvh::MedianPlan med;
    };

    // ---- queries
    bool held() const { return has; }
    bool may_build() const { return !refused && !failed; }   // I2
    bool has_nodes() const { return n_nodes != 0; }
    int why_not() const;                                       // !held(): PT_OK when a host build may be tried, else the refusal of I2
    // ---- operations (stream: the context's; view: its SceneView, whose bvh part only these write)
    void drop(ptk::SceneView& view, bool is_refused, bool is_failed = false);            // the tree is gone (I1), for the reason given (I2)
    int adopt(const ptbvh::Built& b, hipStream_t stream, ptk::SceneView& view);          // upload the host builder's tree; blocking
    int plan(uint32_t n, uint32_t order, const char* who, Rebuild* out) const;           // pure host work; the refusal of a count no tree fits
    int reserve_refit();                                                                 // the box scratch of the held tree
    int reserve_rebuild(const Rebuild& r, ptk::SceneView& view);                         // every array at r's size; a failure leaves no tree (I5); I4
    int upload_plan(Rebuild& r);                                                         // once per count, the stream idle: r.topo, r.med onto the device (I3)
    int enqueue_build(const Rebuild& r, const ptbvh::Bounds& bd, const float4* shape, const uint32_t* tags, hipStream_t stream, ptk::SceneView& view);
    int enqueue_refit(const ptbvh::Bounds& bd, const float4* shape, bool built, hipStream_t stream, ptk::SceneView& view);   // + the cost records (I6)
    int read(const ptk::SceneView& view, const BvhExport& out, uint32_t* out_nodes, uint32_t* out_slots) const;             // blocking; the stream is idle
    int cost(const ptk::SceneView& view, double* cost_now, double* cost_at_build, uint32_t* out_refits) const;              // likewise

private:
    void bind(ptk::SceneView& view, uint32_t root) const;                                 // the four arrays and the root
    static void set_grid(ptk::SceneView& view, const float grid_min[3], const float grid_cell[3], float scene_abs);

    // the tree (I1) and what a refit needs beside it: the nodes by height, scratch for the f32 boxes (2 float4 per leaf slot and node)
    DevBuf<uint4> nodes;
    DevBuf<float4> rec, lead;
    DevBuf<uint32_t> ids, order;
    std::vector<uint32_t> height_first;
    DevBuf<float4> slot_box, node_box;
    uint32_t n_nodes = 0, n_slots = 0, depth = 0;
    bool has = false, refused = false, failed = false;
    // the cost records (I6)
    DevBuf<unsigned long long> cost_sums, cost_built;
    double cost_build = 0.0;
    float cost_cell[3] = {0.f, 0.f, 0.f};
    bool cost_on_device = false;
    uint32_t refits = 0;
    // device builds: the (key, index) pairs and digit histograms of the sort, the cached topology (I3, I4)
    DevBuf<uint2> pairs[2];
    DevBuf<uint32_t> hist;
    struct { DevBuf<uint4> codes; DevBuf<uint32_t> order; std::vector<uint32_t> height_first; int64_t n = -1; uint32_t nodes = 0, slots = 0, root = 0, depth = 0; } topo;
    bool is_morton = false;
    // the median order: the objects' grid cells, the bound words of a level's steps, the cached split plan (I3; its levels here)
    DevBuf<uint2> cells;
    DevBuf<uint32_t> med_bounds, med_groups;
    DevBuf<uint4> med_tiles;
    DevBuf<uint2> med_tsteps;
    std::vector<ptk::BvhMedianLevel> med_levels;
    int64_t med_n = -1;
    uint32_t med_n_tiles = 0, med_index_bits = 0;
};
