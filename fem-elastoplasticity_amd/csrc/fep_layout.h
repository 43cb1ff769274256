// The one definition of every packed table format the host planner (fep_host.h, setup_coo in fep_api.hip) writes and the
// kernels (fep_kernels.hip.h) read: field widths, pack_* / unpack_* / *_fits, the tile record, the LDS image of the P1
// tile kernels, the patch image and the XCD tile order.  Plain C++17 (no HIP include): builds with a host compiler into
// the host test programs (tests/layout_host.cpp checks every function here) and with hipcc into the kernels.
// A format changes HERE and nowhere else: no shift or mask of these words is written out in the planner or a kernel.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define FEP_HD __host__ __device__
#define FEP_UNROLL _Pragma("unroll")
#else
#define FEP_HD
#define FEP_UNROLL
#endif

namespace fep_layout {

constexpr uint32_t field_max(int bits) { return bits >= 32 ? 0xffffffffu : (1u << bits) - 1u; }
FEP_HD constexpr bool in_field(int64_t v, int bits) { return v >= 0 && v <= (int64_t)field_max(bits); }

// ---------------------------------------------------------------------------------------
// Symbolic::meta, one word per node-pair block:  slot:15 | diag:1 | deg:16
//   deg = blocks of the row node, slot = position of the block in its row, diag = row node == column node.
// ---------------------------------------------------------------------------------------
constexpr int kMetaSlotBits = 15, kMetaDiagBits = 1, kMetaDegBits = 16;
constexpr int kMetaDiagShift = kMetaSlotBits, kMetaDegShift = kMetaDiagShift + kMetaDiagBits;
static_assert(kMetaDegShift + kMetaDegBits <= 32, "meta fills at most its word");
struct Meta { int deg, diag, slot; };
FEP_HD constexpr uint32_t pack_meta(uint32_t deg, uint32_t diag, uint32_t slot) { return (deg << kMetaDegShift) | (diag << kMetaDiagShift) | slot; }
FEP_HD constexpr Meta unpack_meta(uint32_t m) {
    return Meta{(int)(m >> kMetaDegShift), (int)((m >> kMetaDiagShift) & field_max(kMetaDiagBits)), (int)(m & field_max(kMetaSlotBits))};
}
FEP_HD constexpr bool meta_fits(int64_t deg, int64_t diag, int64_t slot) {
    return in_field(deg, kMetaDegBits) && in_field(diag, kMetaDiagBits) && in_field(slot, kMetaSlotBits);
}

// ---------------------------------------------------------------------------------------
// Gather code of the P1 kernels:  b:2 | a:2 | i:12 (uint16: slot i of the tile's staged list; P1Plan::codes_pad) or
// i:27 (int32: the element itself; P1Plan::perm2, the direct kernel).  (a, b) = local node pair of the contribution.
// ---------------------------------------------------------------------------------------
constexpr int kGatherNodeBits = 2, kGatherSlotBits = 12, kGatherElemBits = 27;
constexpr int kGatherAShift = kGatherNodeBits, kGatherIShift = 2 * kGatherNodeBits;
static_assert(kGatherIShift + kGatherSlotBits <= 16 && kGatherIShift + kGatherElemBits <= 31, "gather codes fill at most uint16 / a non-negative int32");
struct Gather { int i, a, b; };
FEP_HD constexpr uint32_t pack_gather(uint32_t i, uint32_t a, uint32_t b) { return (i << kGatherIShift) | (a << kGatherAShift) | b; }
FEP_HD constexpr Gather unpack_gather(uint32_t code) {
    return Gather{(int)(code >> kGatherIShift), (int)((code >> kGatherAShift) & field_max(kGatherNodeBits)), (int)(code & field_max(kGatherNodeBits))};
}
FEP_HD constexpr uint32_t gather_ab(uint32_t code) { return code & field_max(kGatherIShift); }          // the (a, b) part, as packed
FEP_HD constexpr bool gather_fits(int64_t i, int64_t a, int64_t b, int i_bits) {
    return in_field(i, i_bits) && in_field(a, kGatherNodeBits) && in_field(b, kGatherNodeBits);
}

// Gather code of the generic node route (GnPlan::codes_pad, uint16):  b:4 | a:4 | i:8
constexpr int kGnNodeBits = 4, kGnSlotBits = 8;
static_assert(2 * kGnNodeBits + kGnSlotBits <= 16, "the generic gather code fills at most uint16");
FEP_HD constexpr uint32_t pack_gn_code(uint32_t i, uint32_t a, uint32_t b) { return (i << (2 * kGnNodeBits)) | (a << kGnNodeBits) | b; }
FEP_HD constexpr Gather unpack_gn_code(uint32_t code) {
    const int a = (int)((code >> kGnNodeBits) & field_max(kGnNodeBits)), b = (int)(code & field_max(kGnNodeBits));
    return Gather{(int)(code >> (2 * kGnNodeBits)), a, b};
}
FEP_HD constexpr bool gn_code_fits(int64_t i, int64_t a, int64_t b) { return in_field(i, kGnSlotBits) && in_field(a, kGnNodeBits) && in_field(b, kGnNodeBits); }

// ---------------------------------------------------------------------------------------
// Packed P1 block descriptor (P1Plan::pkv), one 8-byte load per lane of a tile:
//   x: off:11 | len:4 | deg:8 | slot:8 | diag:1     off / len: the block's gather codes in the tile's code region
//   y: blk:8 | node:8                               block index / index of the row node inside the tile
// ---------------------------------------------------------------------------------------
constexpr int kPkOffBits = 11, kPkLenBits = 4, kPkDegBits = 8, kPkSlotBits = 8, kPkDiagBits = 1, kPkBlkBits = 8, kPkNodeBits = 8;
constexpr int kPkLenShift = kPkOffBits, kPkDegShift = kPkLenShift + kPkLenBits, kPkSlotShift = kPkDegShift + kPkDegBits,
              kPkDiagShift = kPkSlotShift + kPkSlotBits, kPkNodeShift = kPkBlkBits;
static_assert(kPkDiagShift + kPkDiagBits <= 32 && kPkNodeShift + kPkNodeBits <= 32, "pk.x, pk.y fill at most their words");
struct Pk { int off, len, deg, slot, diag, blk, node; };
FEP_HD constexpr uint32_t pack_pk_x(uint32_t off, uint32_t len, uint32_t deg, uint32_t slot, uint32_t diag) {
    return off | (len << kPkLenShift) | (deg << kPkDegShift) | (slot << kPkSlotShift) | (diag << kPkDiagShift);
}
FEP_HD constexpr uint32_t pack_pk_y(uint32_t blk, uint32_t node) { return blk | (node << kPkNodeShift); }
FEP_HD constexpr Pk unpack_pk(uint32_t x, uint32_t y) {
    return Pk{(int)(x & field_max(kPkOffBits)), (int)((x >> kPkLenShift) & field_max(kPkLenBits)), (int)((x >> kPkDegShift) & field_max(kPkDegBits)),
              (int)((x >> kPkSlotShift) & field_max(kPkSlotBits)), (int)(x >> kPkDiagShift),
              (int)(y & field_max(kPkBlkBits)), (int)((y >> kPkNodeShift) & field_max(kPkNodeBits))};
}
FEP_HD constexpr bool pk_fits(const Pk& f) {
    return in_field(f.off, kPkOffBits) && in_field(f.len, kPkLenBits) && in_field(f.deg, kPkDegBits) && in_field(f.slot, kPkSlotBits) &&
           in_field(f.diag, kPkDiagBits) && in_field(f.blk, kPkBlkBits) && in_field(f.node, kPkNodeBits);
}

// ---------------------------------------------------------------------------------------
// Tile record (P1Plan::rec): ONE record of kRecInts int32 (256 bytes) per tile, fetched with scalar loads in one round
// trip at kernel entry (load_tile_rec):
//   [0, kDescInts)    the tile's descriptor (P1Plan::tdesc): [pk_base, n_blocks, head word 0, head word 1], then
//                     kSegMax x [first_block, n_blocks, first_node, n_nodes] (unused segments zero)
//                       head word 0:  nn:8 | n_own:23       nodes of the tile | its first n_own staged elements are its own
//                       head word 1:  nseg:4 | n_el:12 | n_nd:12    segments | staged elements | staged nodes
//   [kRecRng, +16)    the staged elements as <= 8 runs (P1Plan::rng_tab): (start_r, cumulative count_r), see run_entry
//   [kRecNrng, +16)   the staged nodes likewise (P1Plan::nrng_tab)
//   everything else zero; a plan in list form leaves a run part zero: eight runs of cumulative count 0, none live.
// ---------------------------------------------------------------------------------------
constexpr int kSegMax = 4;
constexpr int kDescInts = 4 * (1 + kSegMax);
constexpr int kRecInts = 64, kRecRng = 32, kRecNrng = 48, kRunInts = 16;
static_assert(kDescInts <= kRecRng && kRecRng + kRunInts <= kRecNrng && kRecNrng + kRunInts <= kRecInts, "the tile record's parts do not overlap");
constexpr int kHeadNnBits = 8, kHeadOwnBits = 23, kHeadSegBits = 4, kHeadElBits = 12, kHeadNdBits = 12;
constexpr int kHeadOwnShift = kHeadNnBits, kHeadElShift = kHeadSegBits, kHeadNdShift = kHeadElShift + kHeadElBits;
static_assert(kHeadOwnShift + kHeadOwnBits <= 31 && kHeadNdShift + kHeadNdBits <= 31, "the head words stay non-negative int32");
static_assert(kSegMax <= (int)field_max(kHeadSegBits), "the segment count fits its field");
struct TileHead { int nn, n_own, nseg, n_el, n_nd; };
FEP_HD constexpr int32_t pack_tile_head0(int nn, int n_own) { return nn | (n_own << kHeadOwnShift); }
FEP_HD constexpr int32_t pack_tile_head1(int nseg, int n_el, int n_nd) { return nseg | (n_el << kHeadElShift) | (n_nd << kHeadNdShift); }
FEP_HD constexpr TileHead unpack_tile_head(int32_t w0, int32_t w1) {
    return TileHead{w0 & (int)field_max(kHeadNnBits), w0 >> kHeadOwnShift, w1 & (int)field_max(kHeadSegBits),
                    (w1 >> kHeadElShift) & (int)field_max(kHeadElBits), (w1 >> kHeadNdShift) & (int)field_max(kHeadNdBits)};
}
FEP_HD constexpr bool tile_head_fits(const TileHead& h) {
    return in_field(h.nn, kHeadNnBits) && in_field(h.n_own, kHeadOwnBits) && in_field(h.nseg, kHeadSegBits) &&
           in_field(h.n_el, kHeadElBits) && in_field(h.n_nd, kHeadNdBits);
}
// the head of a descriptor / record in place (d: the tile's kDescInts)
inline TileHead tile_head(const int32_t* d) { return unpack_tile_head(d[2], d[3]); }
inline void set_tile_head(int32_t* d, const TileHead& h) { d[2] = pack_tile_head0(h.nn, h.n_own); d[3] = pack_tile_head1(h.nseg, h.n_el, h.n_nd); }

// Slot i of a list given as <= 8 runs (start_r, cumulative count_r) in r[0 .. 16); slots past the list repeat its first
// entry.  R: const int32_t* (host) or int[16] (the kernels' scalar registers).
template <class R> FEP_HD inline int run_entry(const R& r, int i) {
    int e = r[0] + i;
    FEP_UNROLL
    for (int k = 1; k < 8; ++k) e = i >= r[2 * k - 1] ? r[2 * k] + (i - r[2 * k - 1]) : e;
    return i < r[15] ? e : r[0];
}

// ---------------------------------------------------------------------------------------
// P1Plan::elnodes, one word per staged element of the one-kernel step:  n0:10 | n1:10 | n2:10 | own:1
//   n_a = index of local node a in the tile's staged node list; own = this tile writes the element's point outputs.
// ---------------------------------------------------------------------------------------
constexpr int kElNodeBits = 10, kElOwnShift = 3 * kElNodeBits, kElOwnBits = 1;
static_assert(kElOwnShift + kElOwnBits <= 32, "el_nodes fills at most its word");
struct ElNodes { int n0, n1, n2, own; };
FEP_HD constexpr uint32_t pack_el_nodes(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t own) {
    return n0 | (n1 << kElNodeBits) | (n2 << (2 * kElNodeBits)) | (own << kElOwnShift);
}
FEP_HD constexpr ElNodes unpack_el_nodes(uint32_t w) {
    return ElNodes{(int)(w & field_max(kElNodeBits)), (int)((w >> kElNodeBits) & field_max(kElNodeBits)),
                   (int)((w >> (2 * kElNodeBits)) & field_max(kElNodeBits)), (int)((w >> kElOwnShift) & field_max(kElOwnBits))};
}
FEP_HD constexpr int el_node(uint32_t w, int a) { return (int)((w >> (kElNodeBits * a)) & field_max(kElNodeBits)); }
FEP_HD constexpr bool el_nodes_fits(const ElNodes& f) {
    return in_field(f.n0, kElNodeBits) && in_field(f.n1, kElNodeBits) && in_field(f.n2, kElNodeBits) && in_field(f.own, kElOwnBits);
}

// ---------------------------------------------------------------------------------------
// COO reduce descriptor (csr_reduce_pk_kernel), per block:  x = first contribution,  y: len:8 | deg:12 | slot:12
// ---------------------------------------------------------------------------------------
constexpr int kPkcLenBits = 8, kPkcDegBits = 12, kPkcSlotBits = 12;
constexpr int kPkcDegShift = kPkcLenBits, kPkcSlotShift = kPkcDegShift + kPkcDegBits;
static_assert(kPkcSlotShift + kPkcSlotBits <= 32, "pkc.y fills at most its word");
struct Pkc { int len, deg, slot; };
FEP_HD constexpr uint32_t pack_pkc(uint32_t len, uint32_t deg, uint32_t slot) { return len | (deg << kPkcDegShift) | (slot << kPkcSlotShift); }
FEP_HD constexpr Pkc unpack_pkc(uint32_t y) {
    return Pkc{(int)(y & field_max(kPkcLenBits)), (int)((y >> kPkcDegShift) & field_max(kPkcDegBits)), (int)(y >> kPkcSlotShift)};
}
FEP_HD constexpr bool pkc_fits(const Pkc& f) { return in_field(f.len, kPkcLenBits) && in_field(f.deg, kPkcDegBits) && in_field(f.slot, kPkcSlotBits); }

// ---------------------------------------------------------------------------------------
// Patch route (PatchPlan; element_kernel phase 3, fixup_kernel).
//
// Image: where the phase-3 LDS image keeps the stored block (j, a) of local element el, in 16-byte slots of a plane.
// SKEWED: with the plain (j*n_p + a)*eb + el a step in a is eb slots and a step in j n_p*eb slots — both multiples of 16
// slots = the 256-byte bank row for every element type (eb is a multiple of 8, n_p*eb of 16), so the gather of a CSR row's
// blocks, which walks j and a at fixed el, put all 16 lanes of a `ds_read_b128` group on ONE slot (P4: 49 % of the LDS
// cycles were conflict cycles).  Odd element stride ebp = eb | 1, and one more slot per j when n_p is even, make both
// steps odd.  The force pair (a, el) sits at patch_force_pos of its own region.
//
//   pdesc   kPatchDescInts int32 per patch: item_off, n_items, code_off, n_codes, fitem_off, n_fitems, fcode_off, n_fcodes
//   items   x: off:13 | (cnt-1):6 | deg:12 | open:1    off: code offset in the patch, cnt: contributions (1 .. 64),
//                                                      deg: degree of the row node (closed items)
//           y: closed: position of the block's first row in double2 units (2*nptr[n] + slot); open: partial slot
//   fitems  x: the same word with deg = 0;  y: node | force partial slot
//   codes   uint16  tr:1 | pos:15    pos = patch_image_pos of the stored block, tr = read it transposed;  fcodes  patch_force_pos
//   fix     per upper open block: x = position (as items.y), y: deg:16 | cnt:16, z = first partial slot,
//           w = second partial slot (cnt <= 2) or offset into plist (cnt > 2: `cnt` slots, ascending patch)
//   fixT    its mirror: x = position of the transposed block (kNoMirror: diagonal block), y = degree of ITS row node
//   ffix    per open node:  x = node, y = count, z / w as above
// ---------------------------------------------------------------------------------------
FEP_HD constexpr int patch_ebp(int eb) { return eb | 1; }
FEP_HD constexpr int patch_image_period(int n_p, int eb) { return n_p * patch_ebp(eb) + ((n_p & 1) ? 0 : 1); }      // slots per j
FEP_HD constexpr int patch_image_pos(int n_p, int eb, int j, int a, int el) { return j * patch_image_period(n_p, eb) + a * patch_ebp(eb) + el; }
FEP_HD constexpr int patch_image_slots(int n_p, int eb) { return (n_p / 2 + 1) * patch_image_period(n_p, eb); }
FEP_HD constexpr int patch_force_pos(int eb, int a, int el) { return a * patch_ebp(eb) + el; }
FEP_HD constexpr int patch_force_slots(int n_p, int eb) { return n_p * patch_ebp(eb); }

// Where element_kernel keeps the block (a, b) of K_e: index of the stored block and whether it is the transpose.
// `row_major`: the stored blocks of an element are numbered a*(n_p/2+1) + j (a lane's blocks adjacent: the AoS layout,
// Kc[(e*NB + idx)*4]) instead of j*n_p + a (the SoA layout, Kc[(idx*n_e + e)*4]; the patch image: j = idx / n_p, a = idx % n_p).
FEP_HD inline void sym_block_index(int n_p, int a, int b, int& idx, bool& transposed, bool row_major = false) {
    const int j = b >= a ? b - a : b - a + n_p;
    const bool direct = 2 * j < n_p || (2 * j == n_p && a < n_p / 2);
    const int nj = n_p / 2 + 1;
    if (direct) { idx = row_major ? a * nj + j : j * n_p + a; transposed = false; }
    else { idx = row_major ? b * nj + (n_p - j) : (n_p - j) * n_p + b; transposed = true; }
}
FEP_HD constexpr int sym_block_count(int n_p) { return (n_p / 2 + 1) * n_p; }   // upper bound on idx + 1

constexpr int kPatchDescInts = 8;
constexpr uint32_t kNoMirror = 0xffffffffu;
constexpr int kItemOffBits = 13, kItemCntBits = 6, kItemDegBits = 12, kItemOpenBits = 1;
constexpr int kItemCntShift = kItemOffBits, kItemDegShift = kItemCntShift + kItemCntBits, kItemOpenShift = kItemDegShift + kItemDegBits;
static_assert(kItemOpenShift + kItemOpenBits <= 32, "an item word fills at most its word");
struct PatchItem { int off, cnt, deg, open; };
FEP_HD constexpr uint32_t pack_patch_item(uint32_t off, uint32_t cnt, uint32_t deg, uint32_t open) {
    return off | ((cnt - 1u) << kItemCntShift) | (deg << kItemDegShift) | (open << kItemOpenShift);
}
FEP_HD constexpr PatchItem unpack_patch_item(uint32_t x) {
    return PatchItem{(int)(x & field_max(kItemOffBits)), (int)((x >> kItemCntShift) & field_max(kItemCntBits)) + 1,
                     (int)((x >> kItemDegShift) & field_max(kItemDegBits)), (int)(x >> kItemOpenShift)};
}
FEP_HD constexpr bool patch_item_fits(const PatchItem& f) {
    return in_field(f.off, kItemOffBits) && in_field((int64_t)f.cnt - 1, kItemCntBits) && in_field(f.deg, kItemDegBits) && in_field(f.open, kItemOpenBits);
}

constexpr int kPatchCodePosBits = 15;
static_assert(1 + kPatchCodePosBits <= 16, "a patch code fills at most uint16");
struct PatchCode { int pos, transposed; };
FEP_HD constexpr uint32_t pack_patch_code(uint32_t pos, uint32_t transposed) { return (pos << 1) | transposed; }
// (scalar accessors for phase 3 of element_kernel: through the struct its 512-thread form allocates registers differently)
FEP_HD constexpr uint32_t patch_code_pos(uint32_t code) { return code >> 1; }
FEP_HD constexpr bool patch_code_transposed(uint32_t code) { return code & 1u; }
FEP_HD constexpr PatchCode unpack_patch_code(uint32_t code) { return PatchCode{(int)patch_code_pos(code), (int)patch_code_transposed(code)}; }
FEP_HD constexpr bool patch_code_fits(int64_t pos, int64_t transposed) { return in_field(pos, kPatchCodePosBits) && in_field(transposed, 1); }

constexpr int kFixDegBits = 16, kFixCntBits = 16;
static_assert(kFixDegBits + kFixCntBits <= 32, "fix.y fills at most its word");
struct FixCount { int deg, cnt; };
FEP_HD constexpr uint32_t pack_fix(uint32_t deg, uint32_t cnt) { return deg | (cnt << kFixDegBits); }
FEP_HD constexpr FixCount unpack_fix(uint32_t y) { return FixCount{(int)(y & field_max(kFixDegBits)), (int)(y >> kFixDegBits)}; }
FEP_HD constexpr bool fix_fits(int64_t deg, int64_t cnt) { return in_field(deg, kFixDegBits) && in_field(cnt, kFixCntBits); }

// ---------------------------------------------------------------------------------------
// LDS image of the P1 tile kernels (p1_node_lds_kernel; fused: p1_fused_kernel), byte offsets from the dynamic LDS base.
//   staging:  [0, 15*L doubles) the operands [15][L] | codes: C uint16 | (fused) 16-byte aligned: NL double2 node
//             coordinates, NL double2 node displacements.  With LDS-DMA the code region is padded to 128 codes (64 words)
//             and each node region to 64 entries: a wave's 64 lanes always land inside their region.
//   output:   the same memory afterwards: [0, 2*tile double2) the tile's CSR values | tile double2 nodal forces.
// ---------------------------------------------------------------------------------------
constexpr int kP1Operands = 15;
constexpr int kP1LdsLimit = 96 * 1024;                  // what a plan may ask of a workgroup
// (plans stay below kP1LdsLimit: int holds every offset;  NLp: double2 entries of one node region, nodes_u = nodes_xy + 16 * NLp)
struct P1Lds { int codes, nodes_xy, nodes_u, out_forces, total, NLp; };
FEP_HD constexpr P1Lds p1_tile_lds(int L, int C, int NL, int tile, bool dma, bool fused) {
    const int codes = kP1Operands * L * (int)sizeof(double);
    const int Cp = dma ? (C + 127) & ~127 : C;
    const int NLp = !fused ? 0 : dma ? (NL + 63) & ~63 : NL;
    const int nodes_xy = fused ? (codes + Cp * (int)sizeof(uint16_t) + 15) & ~15 : codes + Cp * (int)sizeof(uint16_t);
    const int nodes_u = nodes_xy + NLp * 16, stage = nodes_u + NLp * 16;
    const int out_forces = tile * 2 * 16, out = out_forces + tile * 16;
    return P1Lds{codes, nodes_xy, nodes_u, out_forces, stage > out ? stage : out, NLp};
}
// LDS of node_lds_kernel (generic node route, measurement build): [9 + 2*n_p][L*n_q] operands, the reference-element tables
// (2 * n_p*n_q + n_q, padded to an even count), then C uint16 codes; returns the offset of the codes / the total.
FEP_HD constexpr size_t gn_lds_codes(int n_p, int n_q, int L) {
    return (size_t)((int64_t)(9 + 2 * n_p) * (L * n_q) + 2 * n_p * n_q + n_q + (n_q & 1)) * sizeof(double);
}
FEP_HD constexpr size_t gn_lds_bytes(int n_p, int n_q, int L, int C) { return gn_lds_codes(n_p, n_q, L) + (size_t)C * sizeof(uint16_t); }

// ---------------------------------------------------------------------------------------
// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (block % 8), each with a private L2.  Every XCD
// gets one contiguous eighth of the tiles, so that the element rows re-staged by the workgroups of the next node row hit
// in the SAME L2 instead of the fabric.  A block whose tile is >= n_wg has none (the grid is rounded up to whole eighths).
// ---------------------------------------------------------------------------------------
constexpr int kXcdBits = 3, kXcds = 1 << kXcdBits;
FEP_HD constexpr int xcd_tile_of_block(unsigned block, int n_wg) {
    const int chunk = (n_wg + kXcds - 1) >> kXcdBits;   // tiles per XCD
    return (int)(block & (unsigned)(kXcds - 1)) * chunk + (int)(block >> kXcdBits);
}
FEP_HD constexpr unsigned xcd_grid(int n_wg) { return (unsigned)(kXcds * ((n_wg + kXcds - 1) / kXcds)); }

}  // namespace fep_layout
