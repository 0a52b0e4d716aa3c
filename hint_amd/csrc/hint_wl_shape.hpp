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

struct WlShape {
    const char* name;
    bool enabled;        // false: the entry stays in the table (and its instances in the library), no launch takes it
    WlFold fwd, bwd;     // training forward, backward part A
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

}  // namespace hint

#include "hint_wl_shape_table.hpp"

namespace hint {
constexpr int WL_N_SHAPES = (int)(sizeof(WL_SHAPES) / sizeof(WL_SHAPES[0]));
// the shape whose constants a launch's arguments equal, or -1
inline int wl_shape_match(const KArgs& a, const WlArgs& w, bool backward) {
    const WlFold f = wl_fold_of(a, w);
    for (int i = 0; i < WL_N_SHAPES; ++i)
        if (WL_SHAPES[i].enabled && wl_fold_equal(f, backward ? WL_SHAPES[i].bwd : WL_SHAPES[i].fwd)) return i;
    return -1;
}
}  // namespace hint
