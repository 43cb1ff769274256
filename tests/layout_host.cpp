// Host-only check of fem-elastoplasticity_amd/csrc/fep_layout.h, the one definition of the table formats the planner packs
// and the kernels unpack.  No argument; prints one line per group of checks; exit code 0 = all hold, 1 = one does not.
//   packed words   every field at its least value, the next, its greatest but one and its greatest, once with all other
//                  fields least and once with all others greatest: unpack(pack(f)) == f, pack sets no bit outside the field
//                  (the fields' masks are disjoint and stay inside the word), *_fits holds at the greatest value of every
//                  field and fails one past it, for each field in turn
//   run_entry      against lists expanded by hand: 1, 2 and 8 runs, slots past the list, the all-zero table of a plan in
//                  list form; as const int32_t* and as int[16]
//   p1_tile_lds    regions in order without overlap, 16-byte alignment, the total against the expression the launchers and
//                  the planner used to write out
//   patch image    patch_image_pos / patch_force_pos injective and inside their slot counts; sym_block_index maps (a, b)
//                  and (b, a) to one stored block with opposite `transposed`
//   XCD order      the blocks of xcd_grid(n) cover the n tiles once each
#include <cstdint>
#include <cstdio>
#include <functional>
#include <set>
#include <vector>

#include "../fem-elastoplasticity_amd/csrc/fep_layout.h"

using namespace fep_layout;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Field { const char* name; int64_t lo, hi; };
struct Format {
    const char* name;
    int bits;                                            // of the word(s): two 32-bit words count as x | y << 32
    std::vector<Field> fields;
    std::function<uint64_t(const int64_t*)> pack;
    std::function<void(uint64_t, int64_t*)> unpack;
    std::function<bool(const int64_t*)> fits;
};

static void check_format(const Format& F) {
    const size_t n = F.fields.size();
    std::vector<int64_t> lo(n), hi(n), x(n), y(n);
    for (size_t i = 0; i < n; ++i) { lo[i] = F.fields[i].lo; hi[i] = F.fields[i].hi; }
    CHECK(F.pack(lo.data()) == 0, "%s", F.name);
    CHECK(F.fits(lo.data()) && F.fits(hi.data()), "%s", F.name);
    const uint64_t all_hi = F.pack(hi.data());
    CHECK(F.bits == 64 || (all_hi >> F.bits) == 0, "%s: bits past the word", F.name);
    uint64_t seen = 0;
    for (size_t f = 0; f < n; ++f) {
        x = lo; x[f] = hi[f];
        const uint64_t mask = F.pack(x.data());          // the greatest value is all ones: the field itself
        CHECK(mask != 0 && (mask & seen) == 0, "%s.%s: overlaps another field", F.name, F.fields[f].name);
        seen |= mask;
        for (const int64_t v : {lo[f], lo[f] + 1, hi[f] - 1, hi[f]}) {
            if (v < lo[f] || v > hi[f]) continue;        // (a one-bit field)
            x = lo; x[f] = v;
            const uint64_t alone = F.pack(x.data());
            F.unpack(alone, y.data());
            CHECK(y == x && (alone & ~mask) == 0, "%s.%s = %lld, others least", F.name, F.fields[f].name, (long long)v);
            x = hi; x[f] = v;
            const uint64_t among = F.pack(x.data());
            F.unpack(among, y.data());
            CHECK(y == x && (among & ~mask) == (all_hi & ~mask) && (among & mask) == alone, "%s.%s = %lld, others greatest", F.name,
                  F.fields[f].name, (long long)v);
            CHECK(F.fits(x.data()), "%s.%s = %lld fits", F.name, F.fields[f].name, (long long)v);
        }
        x = hi; x[f] = hi[f] + 1;
        CHECK(!F.fits(x.data()), "%s.%s: one past the greatest value fits", F.name, F.fields[f].name);
        x = lo; x[f] = lo[f] - 1;
        CHECK(!F.fits(x.data()), "%s.%s: one below the least value fits", F.name, F.fields[f].name);
    }
    CHECK(seen == all_hi, "%s", F.name);
}

static int64_t top(int bits) { return (int64_t)field_max(bits); }

static void check_words() {
    const std::vector<Format> formats = {
        {"meta", 32, {{"deg", 0, top(kMetaDegBits)}, {"diag", 0, 1}, {"slot", 0, top(kMetaSlotBits)}},
         [](const int64_t* v) { return (uint64_t)pack_meta((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]); },
         [](uint64_t w, int64_t* v) { const Meta m = unpack_meta((uint32_t)w); v[0] = m.deg; v[1] = m.diag; v[2] = m.slot; },
         [](const int64_t* v) { return meta_fits(v[0], v[1], v[2]); }},
        {"gather (staged slot)", 16, {{"i", 0, top(kGatherSlotBits)}, {"a", 0, top(kGatherNodeBits)}, {"b", 0, top(kGatherNodeBits)}},
         [](const int64_t* v) { return (uint64_t)pack_gather((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]); },
         [](uint64_t w, int64_t* v) { const Gather g = unpack_gather((uint32_t)w); v[0] = g.i; v[1] = g.a; v[2] = g.b; },
         [](const int64_t* v) { return gather_fits(v[0], v[1], v[2], kGatherSlotBits); }},
        {"gather (element)", 31, {{"i", 0, top(kGatherElemBits)}, {"a", 0, top(kGatherNodeBits)}, {"b", 0, top(kGatherNodeBits)}},
         [](const int64_t* v) { return (uint64_t)pack_gather((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]); },
         [](uint64_t w, int64_t* v) { const Gather g = unpack_gather((uint32_t)w); v[0] = g.i; v[1] = g.a; v[2] = g.b; },
         [](const int64_t* v) { return gather_fits(v[0], v[1], v[2], kGatherElemBits); }},
        {"generic gather", 16, {{"i", 0, top(kGnSlotBits)}, {"a", 0, top(kGnNodeBits)}, {"b", 0, top(kGnNodeBits)}},
         [](const int64_t* v) { return (uint64_t)pack_gn_code((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]); },
         [](uint64_t w, int64_t* v) { const Gather g = unpack_gn_code((uint32_t)w); v[0] = g.i; v[1] = g.a; v[2] = g.b; },
         [](const int64_t* v) { return gn_code_fits(v[0], v[1], v[2]); }},
        {"pk", 64, {{"off", 0, top(kPkOffBits)}, {"len", 0, top(kPkLenBits)}, {"deg", 0, top(kPkDegBits)}, {"slot", 0, top(kPkSlotBits)},
                    {"diag", 0, 1}, {"blk", 0, top(kPkBlkBits)}, {"node", 0, top(kPkNodeBits)}},
         [](const int64_t* v) {
             return (uint64_t)pack_pk_x((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4]) |
                    (uint64_t)pack_pk_y((uint32_t)v[5], (uint32_t)v[6]) << 32;
         },
         [](uint64_t w, int64_t* v) {
             const Pk f = unpack_pk((uint32_t)w, (uint32_t)(w >> 32));
             v[0] = f.off; v[1] = f.len; v[2] = f.deg; v[3] = f.slot; v[4] = f.diag; v[5] = f.blk; v[6] = f.node;
         },
         [](const int64_t* v) { return pk_fits(Pk{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6]}); }},
        {"tile head", 64, {{"nn", 0, top(kHeadNnBits)}, {"n_own", 0, top(kHeadOwnBits)}, {"nseg", 0, top(kHeadSegBits)},
                           {"n_el", 0, top(kHeadElBits)}, {"n_nd", 0, top(kHeadNdBits)}},
         [](const int64_t* v) {
             int32_t d[kDescInts] = {};
             set_tile_head(d, TileHead{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]});
             return (uint64_t)(uint32_t)d[2] | (uint64_t)(uint32_t)d[3] << 32;
         },
         [](uint64_t w, int64_t* v) {
             const int32_t d[kDescInts] = {0, 0, (int32_t)(uint32_t)w, (int32_t)(uint32_t)(w >> 32)};
             const TileHead h = tile_head(d);
             v[0] = h.nn; v[1] = h.n_own; v[2] = h.nseg; v[3] = h.n_el; v[4] = h.n_nd;
         },
         [](const int64_t* v) { return tile_head_fits(TileHead{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]}); }},
        {"el_nodes", 32, {{"n0", 0, top(kElNodeBits)}, {"n1", 0, top(kElNodeBits)}, {"n2", 0, top(kElNodeBits)}, {"own", 0, 1}},
         [](const int64_t* v) { return (uint64_t)pack_el_nodes((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]); },
         [](uint64_t w, int64_t* v) {
             const ElNodes e = unpack_el_nodes((uint32_t)w);
             v[0] = e.n0; v[1] = e.n1; v[2] = e.n2; v[3] = e.own;
             if (el_node((uint32_t)w, 0) != e.n0 || el_node((uint32_t)w, 1) != e.n1 || el_node((uint32_t)w, 2) != e.n2) v[0] = -1;
         },
         [](const int64_t* v) { return el_nodes_fits(ElNodes{(int)v[0], (int)v[1], (int)v[2], (int)v[3]}); }},
        {"pkc", 32, {{"len", 0, top(kPkcLenBits)}, {"deg", 0, top(kPkcDegBits)}, {"slot", 0, top(kPkcSlotBits)}},
         [](const int64_t* v) { return (uint64_t)pack_pkc((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]); },
         [](uint64_t w, int64_t* v) { const Pkc f = unpack_pkc((uint32_t)w); v[0] = f.len; v[1] = f.deg; v[2] = f.slot; },
         [](const int64_t* v) { return pkc_fits(Pkc{(int)v[0], (int)v[1], (int)v[2]}); }},
        {"patch item", 32, {{"off", 0, top(kItemOffBits)}, {"cnt", 1, top(kItemCntBits) + 1}, {"deg", 0, top(kItemDegBits)}, {"open", 0, 1}},
         [](const int64_t* v) { return (uint64_t)pack_patch_item((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]); },
         [](uint64_t w, int64_t* v) { const PatchItem f = unpack_patch_item((uint32_t)w); v[0] = f.off; v[1] = f.cnt; v[2] = f.deg; v[3] = f.open; },
         [](const int64_t* v) { return patch_item_fits(PatchItem{(int)v[0], (int)v[1], (int)v[2], (int)v[3]}); }},
        {"patch code", 16, {{"pos", 0, top(kPatchCodePosBits)}, {"transposed", 0, 1}},
         [](const int64_t* v) { return (uint64_t)pack_patch_code((uint32_t)v[0], (uint32_t)v[1]); },
         [](uint64_t w, int64_t* v) {
             const PatchCode c = unpack_patch_code((uint32_t)w);
             v[0] = c.pos; v[1] = c.transposed;
             if (patch_code_pos((uint32_t)w) != (uint32_t)c.pos || patch_code_transposed((uint32_t)w) != (c.transposed != 0)) v[0] = -1;
         },
         [](const int64_t* v) { return patch_code_fits(v[0], v[1]); }},
        {"fix", 32, {{"deg", 0, top(kFixDegBits)}, {"cnt", 0, top(kFixCntBits)}},
         [](const int64_t* v) { return (uint64_t)pack_fix((uint32_t)v[0], (uint32_t)v[1]); },
         [](uint64_t w, int64_t* v) { const FixCount f = unpack_fix((uint32_t)w); v[0] = f.deg; v[1] = f.cnt; },
         [](const int64_t* v) { return fix_fits(v[0], v[1]); }},
    };
    for (const Format& F : formats) check_format(F);
    CHECK(kNoMirror == 0xffffffffu && kPatchDescInts == 8, "patch constants");
    CHECK(kRecInts * sizeof(int32_t) == 256 && (kRecRng * sizeof(int32_t)) % 64 == 0 && (kRecNrng * sizeof(int32_t)) % 64 == 0, "tile record");
    std::printf("packed words: %zu formats\n", formats.size());
}

static void check_runs() {
    // (start_r, cumulative count_r) x 8; unused runs repeat the first start at the final count (fep_host.h: runs_of)
    struct Case { const char* name; int32_t r[16]; std::vector<int> list; };
    const Case cases[] = {
        {"1 run", {10, 5, 10, 5, 10, 5, 10, 5, 10, 5, 10, 5, 10, 5, 10, 5}, {10, 11, 12, 13, 14}},
        {"2 runs", {10, 3, 20, 5, 10, 5, 10, 5, 10, 5, 10, 5, 10, 5, 10, 5}, {10, 11, 12, 20, 21}},
        {"8 runs", {100, 1, 200, 3, 300, 4, 400, 7, 500, 8, 600, 9, 700, 11, 800, 12},
         {100, 200, 201, 300, 400, 401, 402, 500, 600, 700, 701, 800}},
        {"all zero", {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {}},                // list form: no live run
    };
    for (const Case& c : cases) {
        int regs[16];
        for (int k = 0; k < 16; ++k) regs[k] = c.r[k];
        const int32_t* p = c.r;
        for (int i = 0; i < 300; ++i) {
            const int want = i < (int)c.list.size() ? c.list[(size_t)i] : c.r[0];           // slots past the list: its first entry
            CHECK(run_entry(p, i) == want && run_entry(regs, i) == want, "%s slot %d: %d / %d, expected %d", c.name, i, run_entry(p, i),
                  run_entry(regs, i), want);
        }
    }
    std::printf("run_entry: %zu tables\n", sizeof cases / sizeof cases[0]);
}

static void check_lds() {
    const int sizes[] = {1, 2, 127, 128, 150, 256};
    int n = 0;
    for (int L : sizes) for (int C : sizes) for (int NL : sizes) for (int tile : {128, 256}) for (int fused = 0; fused < 2; ++fused)
        for (int dma = 0; dma <= fused; ++dma) {
            if (C & 1) continue;                         // (the planner pads C to a multiple of 8)
            const P1Lds R = p1_tile_lds(L, C, NL, tile, dma != 0, fused != 0);
            // the expression of the launchers and of the planner's fit test before there was one function
            const size_t Cp = dma ? ((size_t)C + 127) & ~(size_t)127 : (size_t)C;
            const size_t NLp = dma ? ((size_t)NL + 63) & ~(size_t)63 : (size_t)NL;
            const size_t stage = fused ? (((size_t)L * 15 * sizeof(double) + Cp * 2 + 15) & ~(size_t)15) + NLp * 2 * 16
                                       : (size_t)L * 15 * sizeof(double) + (size_t)C * sizeof(uint16_t);
            const size_t out = (size_t)tile * 3 * 16;
            CHECK((size_t)R.total == (stage > out ? stage : out), "L %d C %d NL %d tile %d dma %d fused %d: total %d", L, C, NL, tile, dma, fused, R.total);
            // staging regions, in order: operands, codes, node coordinates, node displacements
            const size_t ends[] = {0, (size_t)15 * L * sizeof(double), (size_t)R.codes + Cp * 2};
            CHECK((size_t)R.codes >= ends[1] && R.codes % 8 == 0, "codes at %d", R.codes);
            if (fused) {
                CHECK((size_t)R.NLp == NLp && (size_t)R.nodes_xy >= ends[2] && (size_t)R.nodes_u >= (size_t)R.nodes_xy + NLp * 16 &&
                      (size_t)R.total >= (size_t)R.nodes_u + NLp * 16, "L %d C %d NL %d dma %d: node regions %d %d of %d", L, C, NL, dma, R.nodes_xy, R.nodes_u, R.total);
                CHECK(R.nodes_xy % 16 == 0 && R.nodes_u % 16 == 0, "node regions at %d %d", R.nodes_xy, R.nodes_u);
                CHECK(!dma || (Cp % 128 == 0 && NLp % 64 == 0), "DMA padding");
            } else {
                CHECK((size_t)R.total >= ends[2], "codes end past the total");
            }
            // output image: 2 * tile double2 of CSR values, tile double2 of forces
            CHECK((size_t)R.out_forces == (size_t)tile * 2 * 16 && R.out_forces % 16 == 0 && (size_t)R.total >= (size_t)R.out_forces + (size_t)tile * 16,
                  "output image: forces at %d of %d", R.out_forces, R.total);
            ++n;
        }
    CHECK(gn_lds_bytes(6, 7, 100, 512) == ((size_t)(9 + 12) * 100 * 7 + 2 * 6 * 7 + 7 + 1) * 8 + 1024 && gn_lds_codes(4, 4, 3) % 8 == 0, "generic node route");
    std::printf("p1_tile_lds: %d shapes\n", n);
}

static void check_patch_image() {
    for (int n_p : {3, 4, 6, 8, 15})
        for (int eb : {8, 16, 28, 60}) {
            const int nj = n_p / 2 + 1, slots = patch_image_slots(n_p, eb);
            std::set<int> seen, fseen;
            for (int j = 0; j < nj; ++j)
                for (int a = 0; a < n_p; ++a)
                    for (int el = 0; el < eb; ++el) {
                        const int pos = patch_image_pos(n_p, eb, j, a, el);
                        CHECK(pos >= 0 && pos < slots && seen.insert(pos).second, "n_p %d eb %d (%d, %d, %d) -> %d of %d", n_p, eb, j, a, el, pos, slots);
                    }
            for (int a = 0; a < n_p; ++a)
                for (int el = 0; el < eb; ++el) {
                    const int pos = patch_force_pos(eb, a, el);
                    CHECK(pos >= 0 && pos < patch_force_slots(n_p, eb) && fseen.insert(pos).second, "n_p %d eb %d force (%d, %d) -> %d", n_p, eb, a, el, pos);
                }
            CHECK(slots == nj * patch_image_period(n_p, eb) && (patch_ebp(eb) & 1) && (patch_image_period(n_p, eb) & 1), "n_p %d eb %d: odd strides", n_p, eb);
        }
    for (int n_p : {3, 4, 6, 8, 15})
        for (int row_major = 0; row_major < 2; ++row_major)
            for (int a = 0; a < n_p; ++a)
                for (int b = 0; b < n_p; ++b) {
                    int i0, i1; bool t0, t1;
                    sym_block_index(n_p, a, b, i0, t0, row_major != 0);
                    sym_block_index(n_p, b, a, i1, t1, row_major != 0);
                    CHECK(i0 >= 0 && i0 < sym_block_count(n_p) && i0 == i1, "n_p %d (%d, %d): blocks %d / %d", n_p, a, b, i0, i1);
                    CHECK(a == b ? (!t0 && !t1) : t0 != t1, "n_p %d (%d, %d): transposed %d / %d", n_p, a, b, (int)t0, (int)t1);
                }
    std::printf("patch image: 5 element types x 4 patch sizes\n");
}

static void check_xcd() {
    for (int n_wg : {1, 7, 8, 9, 1000, 4095}) {
        const unsigned grid = xcd_grid(n_wg);
        CHECK(grid % 8 == 0 && grid >= (unsigned)n_wg && grid < (unsigned)n_wg + 8, "n_wg %d: grid %u", n_wg, grid);
        std::vector<int> hit((size_t)n_wg, 0);
        for (unsigned b = 0; b < grid; ++b) {
            const int t = xcd_tile_of_block(b, n_wg);
            CHECK(t >= 0, "n_wg %d block %u -> %d", n_wg, b, t);
            if (t >= 0 && t < n_wg) ++hit[(size_t)t];
        }
        for (int t = 0; t < n_wg; ++t) CHECK(hit[(size_t)t] == 1, "n_wg %d: tile %d taken %d times", n_wg, t, hit[(size_t)t]);
    }
    std::printf("XCD order: 6 grids\n");
}

int main() {
    check_words();
    check_runs();
    check_lds();
    check_patch_image();
    check_xcd();
    std::printf("result %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
