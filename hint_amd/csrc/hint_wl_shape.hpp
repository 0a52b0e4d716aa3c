// Shape policy of the wave-local row kernels (hint_wl.hpp): which fields of KArgs / WlArgs depend on nothing but (tree
// shape, plan variant, wavefronts per workgroup, row tiles per workgroup) - and may therefore be compile-time constants of a
// kernel instance - and the table of shapes that have such instances (hint_wl_shape_table.hpp, printed by
// tools/wl_shape_table.py from the planner: never typed by hand).
//
// The kernels take the policy as a trailing template parameter pack:
//   <>                 the dynamic instance: every field is the kernel argument (the only instance there was)
//   <WlStatic<ID>>     shape ID of the table: the fields below are constants of the instance; the launch site
//                      (hint_abi.cpp row_launch) picks it only when EVERY one of them equals the launch's own value,
//                      compared field by field - anything else runs the dynamic instance.
// Everything that scales with the batch (B, a2_off, bits_off, bits_stride, act_stride, thin_slab_off), alpha, the chain length
// and all pointers stay kernel arguments; row records, slot tables and ranges stay data.
//
// The LEVEL SCHEDULE is a second set of constants (WlSched): per group of the plan what the group loop, the rows and the coupling
// otherwise read from tables in every block of the chain although the shape fixes it - the group's entries and level, the
// backward boundary's slot count, and the fields that are the same in EVERY row record of the group (k-blocks, first-layer
// widths, hidden width, smallest / largest tile count, how many wavefronts share a unit).  The planner derives it by walking
// every record of the group (hint_plan.cpp wl_sched_of); a field that is not uniform over the group is -1 there, which no table
// entry holds - the generator refuses to print one - so such a plan runs the dynamic instance.
#pragma once
#include "hint_dev.h"

namespace hint {

// folded fields of KArgs (X(name)) and of WlArgs (Y(name)); one list for the table's record, the generator's export,
// the host's comparison and the kernels' fold
#define HINT_WL_FOLD_K(X)                                                                                             \
    X(d) X(dc) X(xld) X(gld) X(n_groups) X(n_levels) X(n_units) X(nw) X(WT) X(ST) X(total_rows) X(meta_bytes)         \
    X(units_off) X(tmap_off) X(ents_off) X(rng_off) X(lops_off) X(lop_cnt) X(tw_floats) X(fuse_dw1) X(lean)           \
    X(perm_lds) X(thin_lds)
#define HINT_WL_FOLD_W(Y)                                                                                             \
    Y(par_f4) Y(par_bias) Y(bias_src) Y(off_par) Y(off_slab) Y(slab_floats) Y(off_perm) Y(off_priv) Y(priv_stride)    \
    Y(priv_tile) Y(off_misc) Y(off_recs) Y(nr)

struct WlFold {          // one direction's constants
#define X(f) int32_t a_##f;
#define Y(f) int32_t w_##f;
    HINT_WL_FOLD_K(X)
    HINT_WL_FOLD_W(Y)
#undef X
#undef Y
};
#define X(f) +1
constexpr int WL_FOLD_FIELDS = 0 HINT_WL_FOLD_K(X) HINT_WL_FOLD_W(X);
#undef X
static_assert(WL_FOLD_FIELDS == 36, "HINT_WL_FOLD_FIELDS of include/hint_amd.h");
static_assert(sizeof(WlFold) == 4 * WL_FOLD_FIELDS, "WlFold is WL_FOLD_FIELDS int32 in list order (hint_plan_check_wl_shape copies it out as such)");

// one group's schedule constants (Z(name)); groups in the plan's order (the forward runs them 0 .. n_groups - 1, the backward back)
#define HINT_WL_GROUP_K(Z)                                                                                            \
    Z(ent_begin) Z(ent_cnt) Z(level) Z(level_last) Z(slots) Z(n1) Z(ntt_min) Z(ntt_max) Z(thin_K) Z(cin) Z(kcp) Z(hw) Z(sl)
constexpr int WL_MAX_G = 4;         // groups of a plan with a schedule (more: the schedule is invalid, the launch dynamic)
struct WlGroupK {
    int32_t ent_begin, ent_cnt;     // the group's coupling entries (Group)
    int32_t level, level_last;
    int32_t slots;                  // backward: slots of the boundary in front of the group (ranges table at lop_cnt)
    int32_t n1;                     // k-blocks of every row of the group
    int32_t ntt_min, ntt_max;       // smallest / largest tile count of its rows
    int32_t thin_K;                 // inputs of the thin layer in front of the rows: thin_k & 0xff (forward cin, backward r)
    int32_t cin, kcp, hw;           // first-layer inputs, their padded count in the dW1 slab (4 or 8), hidden width of every unit
    int32_t sl;                     // wavefronts that share a unit = slabs per net that the coupling / the scatter add up
};
struct WlSched {                    // one direction's schedule; unused groups are zero
    WlGroupK g[WL_MAX_G];
    int32_t tail_slots;             // backward: slots of the boundary behind group 0
};
#define Z(f) +1
constexpr int WL_GROUP_FIELDS = 0 HINT_WL_GROUP_K(Z);
#undef Z
constexpr int WL_SCHED_FIELDS = WL_MAX_G * WL_GROUP_FIELDS + 1;
static_assert(WL_GROUP_FIELDS == 13 && WL_SCHED_FIELDS == 53, "HINT_WL_SCHED_FIELDS of include/hint_amd.h");
static_assert(sizeof(WlSched) == 4 * WL_SCHED_FIELDS, "WlSched is WL_SCHED_FIELDS int32 in list order (hint_plan_check_wl_shape copies it out as such)");

struct WlShape {
    const char* name;
    bool enabled;        // false: the entry stays in the table (and its instances in the library), no launch takes it
    WlFold fwd, bwd;     // training forward, backward part A
    WlSched sfwd, sbwd;  // their level schedules
};

template <int ID> struct WlStatic { static constexpr int id = ID; };

inline WlFold wl_fold_of(const KArgs& a, const WlArgs& w) {
    WlFold f{};
#define X(n) f.a_##n = a.n;
#define Y(n) f.w_##n = w.n;
    HINT_WL_FOLD_K(X)
    HINT_WL_FOLD_W(Y)
#undef X
#undef Y
    return f;
}
inline bool wl_fold_equal(const WlFold& p, const WlFold& q) {
    bool same = true;
#define X(n) same = same && p.a_##n == q.a_##n;
#define Y(n) same = same && p.w_##n == q.w_##n;
    HINT_WL_FOLD_K(X)
    HINT_WL_FOLD_W(Y)
#undef X
#undef Y
    return same;
}
inline bool wl_sched_equal(const WlSched& p, const WlSched& q) {
    bool same = p.tail_slots == q.tail_slots;
    for (int i = 0; i < WL_MAX_G; ++i) {
#define Z(n) same = same && p.g[i].n == q.g[i].n;
        HINT_WL_GROUP_K(Z)
#undef Z
    }
    return same;
}
// a schedule the kernels may fold: every field of every group is uniform (none is -1)
constexpr bool wl_sched_valid(const WlSched& p, int n_groups) {
    bool ok = n_groups >= 1 && n_groups <= WL_MAX_G && p.tail_slots >= 0;
    for (int i = 0; ok && i < n_groups; ++i) {
#define Z(n) ok = ok && p.g[i].n >= 0;
        HINT_WL_GROUP_K(Z)
#undef Z
    }
    return ok;
}

}  // namespace hint

#include "hint_wl_shape_table.hpp"

namespace hint {
constexpr int WL_N_SHAPES = (int)(sizeof(WL_SHAPES) / sizeof(WL_SHAPES[0]));
// the shape whose constants a launch's arguments and its plan's level schedule equal, or -1
inline int wl_shape_match(const KArgs& a, const WlArgs& w, const WlSched& s, bool backward) {
    const WlFold f = wl_fold_of(a, w);
    if (!wl_sched_valid(s, a.n_groups)) return -1;
    for (int i = 0; i < WL_N_SHAPES; ++i)
        if (WL_SHAPES[i].enabled && wl_fold_equal(f, backward ? WL_SHAPES[i].bwd : WL_SHAPES[i].fwd) &&
            wl_sched_equal(s, backward ? WL_SHAPES[i].sbwd : WL_SHAPES[i].sfwd)) return i;
    return -1;
}
}  // namespace hint
