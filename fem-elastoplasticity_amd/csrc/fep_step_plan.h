// Which kernels a step launches, decided once and as data: plan_step(facts, wants) is the one decision that the runner
// (fep_api.hip, run_step), the scratch allocator (ensure_scratch) and the name printer (fep_ctx_kernel_names) read.
// Plain C++17 (no HIP include, no allocation): builds with a host compiler into tests/step_plan_host.cpp, which walks
// every StepFacts x StepWants, and with hipcc into the library.
#pragma once
#include <cstdint>

namespace fep_plan {

// What a context runs, chosen once at creation (fep_api.hip, choose_route):
//   P1Node   P1's node route: p1_point_kernel + p1_node_lds_kernel, or p1_fused_kernel alone (K,F-only steps)
//   Patch    element_kernel in its patch form (K_e summed in LDS) + fixup_kernel: every other type, P1 with FEP_ROUTE=patch
//   Coo      element_kernel with every K_e block through HBM + csr_reduce*: FEP_ROUTE=coo, or a mesh without a patch plan
//   GenNode  (only the -DFEP_ABLATION build creates it, FEP_GEN_PATH=node) P2 / Q1 / Q2: point_kernel + node_lds_kernel
enum class Route : uint8_t { P1Node, Patch, Coo, GenNode };

// What of a context the decision reads
struct StepFacts {
    Route route = Route::Coo;
    bool dp = true;                 // the model is Drucker-Prager
    // P1Node (the product's plan: lds, fused_mode 1, !asm_from_nodes)
    bool lds = true;                // LDS-staged tile kernel (false: the direct kernel)
    bool fused = false;             // the context has the one-kernel step's tables
    int fused_mode = 1;             // 0 = never the one-kernel step, 1 = only when no point output is wanted, 2 = always
    bool asm_from_nodes = false;    // assembly by the one-kernel step's assembly-only form
    // Coo
    bool pkc = true;                // packed block descriptors (csr_reduce_pk_kernel)
};

// What a call asks for.  `assemble`: fep_assemble_dev, whose ds / s are the caller's inputs (the point outputs stay false)
struct StepWants {
    bool accept = false;
    bool e = false, s = false, ds = false, ind_p = false;
    bool K = false, F = false, counts = false;
    bool field = false;
    bool assemble = false;
};

// Stage A, in front of mark 1: the model's point kernel; the element kernel from U (Drucker-Prager's whole element-route
// step) or from ds / s (fep_assemble_dev on the element routes); GenNode's point kernel
enum class StageA : uint8_t { None, Point, ElementFromU, ElementFromDs, GenPoint };
// Stage B, between marks 1 and 2.  P1Node: the one-kernel step, the tile kernel, the direct kernel, the assembly-from-nodes
// form; Patch: fix-up; Coo: reduce with packed / unpacked descriptors; GenNode: node_lds_kernel
enum class StageB : uint8_t { None, OneKernel, Tile, Direct, FromNodes, Fixup, ReducePk, Reduce, GenNode };
// Which launch sums the branch counters: stage B itself, counts_finalize_kernel behind the one-kernel step (in front of
// mark 2), or counts_reduce_kernel behind mark 3
enum class CountSum : uint8_t { None, StageB, Finalize, Reduce };
// Where they were written, which is how many entries the sum reads: blk_counts by the route's stage-A grid or by the point
// kernel's grid, or the one-kernel step's slot counters
enum class CountGrid : uint8_t { None, RouteStageA, PointKernel, Slots };
// The internal ds / s arrays that carry the point stage's results to the assembly
struct Scratch {
    bool ds = false, s = false;
};
constexpr Scratch operator|(Scratch a, Scratch b) { return Scratch{a.ds || b.ds, a.s || b.s}; }
constexpr bool covers(Scratch have, Scratch need) { return (have.ds || !need.ds) && (have.s || !need.s); }

struct StepPlan {
    StageA a = StageA::None;
    bool elem_assembly = false;     // behind mark 1, in front of stage B: element_kernel in its assembly-only form (staged steps)
    StageB b = StageB::None;
    bool force_gather = false;      // stage C, between marks 2 and 3: the COO form's force gather
    CountSum sum = CountSum::None;
    CountGrid grid = CountGrid::None;
    Scratch use;                    // the internal array stands in for the caller's ds / s
    Scratch need;                   // what must exist before the launches (a staged step asks for both, as it always has)
    bool lazy = false;              // `need` is allocated by the first such call, not by set_materials / set_model
};

constexpr bool element_route(Route r) { return r == Route::Patch || r == Route::Coo; }
// Every model but Drucker-Prager, and every model with a field, runs staged: point kernel, then what fep_assemble_dev launches
constexpr bool staged(const StepFacts& f, const StepWants& w) { return !w.assemble && (!f.dp || w.field); }
// The one-kernel step: Drucker-Prager without a field, not accepting, K or F wanted, point outputs only in mode 2
constexpr bool one_kernel(const StepFacts& f, const StepWants& w) {
    const bool point_outputs = w.e || w.s || w.ds || w.ind_p;
    return f.route == Route::P1Node && f.dp && !w.field && !w.assemble && f.fused && !w.accept && (w.K || w.F) &&
           f.fused_mode > (point_outputs ? 1 : 0);
}

// Stage B of a route when K and / or F are assembled (`counts`: the fix-up launch also runs for the counter sum alone)
constexpr StageB assembly_stage(const StepFacts& f, bool K, bool F, bool counts) {
    switch (f.route) {
        case Route::P1Node: return !(K || F) ? StageB::None : (f.fused && f.asm_from_nodes) ? StageB::FromNodes : f.lds ? StageB::Tile : StageB::Direct;
        case Route::GenNode: return K || F ? StageB::GenNode : StageB::None;
        case Route::Patch: return K || F || counts ? StageB::Fixup : StageB::None;
        case Route::Coo: return !K ? StageB::None : f.pkc ? StageB::ReducePk : StageB::Reduce;
    }
    return StageB::None;
}
// (the direct kernel is the one assembly kernel that cannot sum the counters on the side)
constexpr bool sums_counters(StageB b) { return b != StageB::None && b != StageB::Direct; }

constexpr StepPlan plan_step(const StepFacts& f, const StepWants& w) {
    StepPlan p;
    const bool er = element_route(f.route);
    if (w.assemble) {                                   // from the caller's ds / s: no stage reads U, nothing counts
        p.a = er ? StageA::ElementFromDs : StageA::None;
        p.b = assembly_stage(f, w.K, w.F, false);
        p.force_gather = f.route == Route::Coo && w.F && !w.K;
        return p;
    }
    if (one_kernel(f, w)) {
        p.b = StageB::OneKernel;
        if (w.counts) { p.sum = CountSum::Finalize; p.grid = CountGrid::Slots; }
        return p;
    }
    const bool stg = staged(f, w);
    // a two-kernel step passes ds / s from the point kernel to the assembly through HBM
    if (stg || !er) p.use = Scratch{w.K && !w.ds, w.F && !w.s};
    p.need = stg ? Scratch{true, true} : p.use;
    // allocated on first use: a Drucker-Prager field step, and a Drucker-Prager step that the one-kernel context's tables
    // could not take (accepting, or with point outputs; such a context keeps no scratch until then)
    p.lazy = f.dp && (w.field || (f.route == Route::P1Node && f.fused && f.fused_mode >= 1));
    if (stg) {
        p.a = StageA::Point;
        p.elem_assembly = er && (w.K || w.F);
        p.b = assembly_stage(f, w.K, w.F, false);       // (stage B gets no counters: the point kernel's are summed behind mark 3)
        if (w.counts) { p.sum = CountSum::Reduce; p.grid = CountGrid::PointKernel; }
    } else {
        p.a = er ? StageA::ElementFromU : f.route == Route::GenNode ? StageA::GenPoint : StageA::Point;
        p.b = assembly_stage(f, w.K, w.F, w.counts);
        if (w.counts) { p.sum = sums_counters(p.b) ? CountSum::StageB : CountSum::Reduce; p.grid = CountGrid::RouteStageA; }
    }
    p.force_gather = f.route == Route::Coo && w.F && !w.K;
    return p;
}

// The 2^10 calls a context can get
constexpr int kWantsCount = 1 << 10;
constexpr StepWants wants_of(int i) {
    auto bit = [i](int k) { return ((i >> k) & 1) != 0; };
    return StepWants{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), bit(9)};
}
// What set_materials / set_model allocate: the union of the scratch of every plan that is not lazy, so that no such step
// allocates (a step may run inside a stream capture, where allocating is refused)
constexpr Scratch prealloc_scratch(const StepFacts& f) {
    Scratch all;
    for (int i = 0; i < kWantsCount; ++i) {
        const StepPlan p = plan_step(f, wants_of(i));
        if (!p.lazy) all = all | p.need;
    }
    return all;
}

}  // namespace fep_plan
