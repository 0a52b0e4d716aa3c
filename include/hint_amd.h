/* hint_amd.h — C ABI of the MI355X (gfx950) implementation of HINT's recursive
 * affine-coupling block: forward / inverse / log|det J| and the backward pass.
 *
 * This is the drop-in boundary.  The reference (vislearn/HINT) has no native code; the
 * interface replaced here is the Python module protocol of
 *     /root/reference/hint.py:104-133   HierarchicalAffineCouplingBlock
 *         .forward(x:list, c=[], rev=False) -> [Tensor]      (hint.py:124-126)
 *         .jacobian(x, c=[], rev=False)     -> Tensor[B]     (hint.py:128-129)
 *     /root/reference/hint.py:21-101    HierarchicalAffineCouplingTree (the arithmetic)
 * plus the autograd backward PyTorch derives from it when the training loop calls
 * loss.backward() (/root/reference/train_unconditional.py:137).
 * `hint_amd/hint.py` is the host-side mirror of that module and binds these symbols with
 * ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success, non-zero on error
 *     (hint_last_error() gives a thread-local message); no exceptions cross the boundary.
 *   - all tensors are fp32, row-major, caller-allocated DEVICE memory: x,z,g_x,g_z [B,d];
 *     c,g_c [B,dc] (all conditions concatenated, hint.py:76); J,g_J [B].
 *   - calls are asynchronous and ordered on `stream` (a hipStream_t passed as void*).
 *   - a plan is immutable after creation and bound to the HIP device current at creation;
 *     it may be shared by threads.  Parameters are passed per call as ONE flat fp32 buffer
 *     whose layout the caller described at plan creation (p_off, in floats), because the
 *     reference loops rebind p.data / call .to() (train_unconditional.py:165-167).
 *   - outputs, tapes, workspaces and packed buffers need no initialisation: only buffers documented
 *     as accumulated (g_params with accumulate != 0, loss_acc) are read before they are written
 *     (tests/test_gpu_poison.py runs every entry point on NaN- and junk-filled memory).
 */
#ifndef HINT_AMD_H
#define HINT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HINT_AMD_ABI_VERSION 8

/* index into hint_node_desc.p_off: [net][tensor]; net 0 = s, net 1 = t (hint.py:44-45);
 * tensors in nn.Sequential order (hint.py:11-13): W1 [h,cin], b1 [h], W2 [h,h], b2 [h],
 * W3 [r,h], b3 [r]; all row-major [out,in] like torch.nn.Linear.weight. */
enum { HINT_W1 = 0, HINT_B1 = 1, HINT_W2 = 2, HINT_B2 = 3, HINT_W3 = 4, HINT_B3 = 5 };

/* One node of the coupling tree (hint.py:25-54), in any order.  A node owns lanes
 * [off, off+D); its first k lanes condition the transform of the other r = D-k >= 1
 * (hint.py:41,68 always split at k = D/2; other splits are accepted, e.g. k = 0 for a coupling
 * that transforms all its lanes given the condition only, conditional_hint_4_full.py:76-82).
 * depth = 0 for the root.  Nodes of equal depth own disjoint lanes. */
typedef struct hint_node_desc {
    int32_t off, D, k, r;
    int32_t h;          /* hidden width of both subnets (hint.py:44-45) */
    int32_t depth;
    int64_t p_off[12];  /* offsets in floats into the flat parameter buffer: [net*6 + tensor] */
} hint_node_desc;

typedef struct hint_plan hint_plan;

/* Build the static level schedule for one block.  d = lanes of the block, dc = total
 * condition width (0 if unconditional), clamp as in hint.py:108 (alpha = clamp*0.636,
 * hint.py:57,60).  Replaces HierarchicalAffineCouplingTree.__init__ (hint.py:25-54). */
int hint_plan_create(const hint_node_desc* nodes, int32_t n_nodes, int32_t d, int32_t dc,
                     float clamp, hint_plan** out);

/* Host-only dry run of hint_plan_create (no device needed, nothing uploaded): builds the plan, lets the
 * planner verify its own schedule (every fragment tile of every group in exactly one wavefront's range of
 * either GEMM phase, slices and slabs consistent with the ranges) and reports what it came to:
 * stats[16] = { groups, levels, WT (activation columns), ST (coupling-gradient columns), LDS bytes forward,
 * LDS bytes backward, wavefronts per workgroup, part-B tile jobs, parameter floats, packed floats, units,
 * fragment tiles of the widest group, subtree groups (the deepest levels that run one subtree per wavefront; 0: none),
 * 1 when the block runs on the wave-local kernels, single-tile part-B jobs that share workgroups,
 * slots (threads per batch row) of the backward's widest boundary }.
 * For tests and tools; same return convention as hint_plan_create. */
int hint_plan_check(const hint_node_desc* nodes, int32_t n_nodes, int32_t d, int32_t dc, float clamp,
                    int64_t* stats);
void hint_plan_destroy(hint_plan* plan);

/* floats the flat parameter (and gradient) buffer must hold: max(p_off + tensor size), rounded up to 4. */
/* (A plan may hold two launch variants of the block - 8 wavefronts per workgroup for batches of up to one 16-row tile
 * per CU, 4 for larger ones - and every entry point that takes B picks by B; the sizes below are the picked
 * variant's, so query them with the B you will run.) */
int64_t hint_plan_param_floats(const hint_plan* plan);
/* floats of the packed-weight buffer (both subnets of every node, forward and transposed
 * copies, in MFMA fragment order, zero padded, and 1024 floats of zeros at the end); the pack writes
 * every float of it. */
int64_t hint_plan_packed_floats(const hint_plan* plan);
/* floats of the forward "tape" for a batch of B rows, recorded by the training forward and read
 * by the backward pass: per tree level one [B,d] snapshot of the lane tensor as that level saw it
 * (the last slice holds the block's permuted input for the _ex / chain forms) and one [B,d] array
 * of the level's coupling arguments s (indexed by the lane each one scales); the hidden activations
 * a2 of every subnet, [B rounded up to 16, sum of 2*pad16(h)] (and a1, the same size, unless every
 * subnet of the block has 1..4 inputs, at most 4 outputs and no condition; tree levels of that kind -
 * "lean" groups - leave their a1 columns unwritten in any case: a1 is rebuilt where it is needed); and one sign byte per four activations (what the backward kernel reads instead
 * of the activations).  The backward pass recomputes nothing else (what autograd keeps for hint.py:77,
 * minus the pre-activations), and the weight-gradient kernel takes its a2 / lane operands from here. */
int64_t hint_plan_tape_floats(const hint_plan* plan, int32_t B);
/* bytes of scratch hint_block_backward needs for a batch of B rows: the per-row gradient factors g1, g2
 * ([B rounded up to 16, sum of 2*pad16(h)] each; neither for lean plans, whose backward kernel computes the
 * first-layer gradients itself into one small slab per workgroup) and g_s | g_t, and one partial-gradient
 * slab per batch split of the weight-gradient kernel. */
size_t hint_plan_workspace_bytes(const hint_plan* plan, int32_t B);
/* dynamic LDS bytes per workgroup of the forward / backward kernels (informational). */
int32_t hint_plan_lds_bytes(const hint_plan* plan, int32_t backward);
/* Which kernels a batch of B rows runs on (diagnostics, bench labels): out[0] = 1 when the block runs on the wave-local
 * kernels (hint_wl_apply_kernel / hint_wl_bwd_kernel: every subnet has 1..4 inputs and at most 4 outputs), 0 for the
 * general ones (hint_apply_kernel / hint_bwd_kernel); out[1] = 16-row tiles per workgroup (1, or 2: row pairs);
 * out[2] = wavefronts per workgroup; out[3] = 1 when no a1 / g2 arrays exist (part B rebuilds them); out[4] = subtree groups (the
 * deepest levels that run one subtree per wavefront); out[5] = tiles of the widest row (<= 3: the general backward pass runs on
 * hint_bwd_kernel_n3, unless out[6]); out[6] = 1 when rows of the backward kernel compute first-layer weight gradients themselves;
 * out[7] = 1 when some general group is lean: forward and inverse run on hint_apply_kernel<REV, true>, whose rows make such groups'
 * first layer themselves (no thin phase), else on hint_apply_kernel<REV, false>.  out must hold 8 values. */
int hint_plan_describe(const hint_plan* plan, int32_t B, int32_t* out);

/* The launch decision for a batch of B >= 1 rows, as the entry points take it (one function decides for hint_block_forward*,
 * hint_block_inverse*, hint_block_backward* and the chain's forward, inverse and backward): which compiled kernel instance every
 * launch runs on and how often its tile loop `for (tg = blockIdx.x; tg < groups; tg += gridDim.x)` goes round.  Writes the first
 * min(n_out, HINT_DISPATCH_FIELDS) of:
 *   [0] 1: wave-local kernels (hint_wl_apply_kernel<REV, NR, CH> / hint_wl_bwd_kernel<NR, CH>), 0: general ones
 *   [1] NR, 16-row tiles per workgroup (2: row pairs)        [2] wavefronts per workgroup
 *   [3] 1 when the batch runs on the plan's 4-wavefront variant
 *   [4] 16-row tiles    [5] tile groups (ceil(tiles / NR))    [6] workgroups of the row kernels    [7] passes (ceil(groups / grid))
 *   [8] forward / inverse: 0 hint_wl_apply_kernel, 1 hint_apply_kernel<REV, false>, 2 hint_apply_kernel<REV, true>
 *   [9] backward part A: 0 hint_wl_bwd_kernel, 1 hint_bwd_kernel, 2 hint_bwd_kernel_n3, 3 hint_bwd_kernel_fly
 *   [10] [11] part B: S and W of hint_wgrad_kernel<S, W>      [12] [13] part B's batch splits and rows per split (one block)
 *   [14] subtree groups    [15] lean    [16] some group is lean-wide    [17] rows of the backward kernel compute dW1 | db1 (rowdw)
 *   [18] first-layer weight gradients come from the backward kernel (fuse_dw1)    [19] CUs the decision assumed.
 * CH (chained launch or single block) is the entry point's, not part of the decision. */
#define HINT_DISPATCH_FIELDS 20
int hint_plan_dispatch(const hint_plan* plan, int32_t B, int32_t* out, int32_t n_out);
/* The same for a host-only plan (as hint_plan_check builds it: no device needed) on a device of num_cu CUs. */
int hint_plan_check_dispatch(const hint_node_desc* nodes, int32_t n_nodes, int32_t d, int32_t dc, float clamp, int32_t B,
                             int32_t num_cu, int32_t* out, int32_t n_out);
/* Which of the planner's attempts a plan came from and how it stages its tables, for the variant a batch of B >= 1 rows runs on (the
 * planner tries smaller groups, then fewer wavefronts per unit, until the block fits the LDS; thresholds decide what rides in LDS).
 * Writes the first min(n_out, HINT_PATH_FIELDS) of:
 *   [0] fragment tiles per group the accepted attempt allowed (64, 48, 32 or 16)
 *   [1] wavefronts that may share one unit's rows in the accepted attempt (the variant's wavefront count, halved down to 1)
 *   [2] groups    [3] tree levels
 *   [4] the thin layers' vectors, forward: 0 read from L2, 1 the whole blob staged in LDS, 2 one group's slice at a time
 *   [5] the same, backward
 *   [6] 1 when, in mode 2, some group's slice is larger than the buffer and that group reads from L2 (forward)    [7] backward
 *   [8] the backward's slot table: 1 in LDS, 0 in global memory
 *   [9] 1 when rows of the backward kernel compute dW1 | db1 (rowdw)
 *   [10] tail tiles (16 outputs each) of the widest r    [11] tail tiles (16 inputs each) of the widest cin.
 * Reported only: no kernel and no launch reads these values, and they are no part of hint_plan_check_digest. */
#define HINT_PATH_FIELDS 12
int hint_plan_paths(const hint_plan* plan, int32_t B, int32_t* out, int32_t n_out);
/* The same for a host-only plan (as hint_plan_check builds it: no device needed) on a device of num_cu CUs. */
int hint_plan_check_paths(const hint_node_desc* nodes, int32_t n_nodes, int32_t d, int32_t dc, float clamp, int32_t B,
                          int32_t num_cu, int32_t* out, int32_t n_out);
/* Host-only as well: the shape-specialised instances of the wave-local row kernels (hint_amd/csrc/hint_wl_shape.hpp).  For a
 * CHAINED training launch (backward = 0: forward, 1: backward part A) of B >= 1 rows on a device of num_cu CUs, with
 * (with_perm = 1) or without fixed permutations between the blocks, returns
 *   field -1: the entry of the shape table whose instance the launch takes (every folded field equal), or -1: the dynamic instance
 *   field 0 .. HINT_WL_FOLD_FIELDS - 1: the launch's own folded field of that index, in the order of that header's field lists
 *             (tools/wl_shape_table.py prints the table from them).
 *   field HINT_WL_SCHED_FIELD0 + i, i < HINT_WL_SCHED_FIELDS: int32 i of the launch's level schedule (that header's WlSched: per
 *             group of the plan, up to four, its thirteen schedule constants in list order, then the backward's tail slot count),
 *             derived by walking every row record of the group; a field that is not the same in every record of its group is -1,
 *             and a launch whose schedule holds one takes the dynamic instance.
 * A plan that does not run on the wave-local kernels reports -1 and zeros.  INT64_MIN (and hint_last_error) on bad arguments. */
#define HINT_WL_FOLD_FIELDS 36
#define HINT_WL_SCHED_FIELD0 1000
#define HINT_WL_SCHED_FIELDS 53
int64_t hint_plan_check_wl_shape(const hint_node_desc* nodes, int32_t n_nodes, int32_t d, int32_t dc, float clamp, int32_t B,
                                 int32_t num_cu, int32_t backward, int32_t with_perm, int32_t field);
/* Host-only as well: one 64-bit digest per table the planner emits, first for the plan, then for its 4-wavefront variant (zeros
 * when there is none).  Per plan HINT_PLAN_DIGESTS values: meta blob, slot table, thin records, row records, bias map, real-element
 * map, weight-gradient jobs, first-layer-gradient map, pack segments, pack tiles, unit_w23, the plan's scalar fields.  Writes the
 * first n_out of the 2 * HINT_PLAN_DIGESTS values.  tests/test_plan_digest_cpu.py pins them: a planner change shows which table moved. */
#define HINT_PLAN_DIGESTS 12
int hint_plan_check_digest(const hint_node_desc* nodes, int32_t n_nodes, int32_t d, int32_t dc, float clamp, uint64_t* out,
                           int32_t n_out);
/* Host-only as well: part B's launch list of the plan (variant 0) or of its 4-wavefront variant (1) - the weight-gradient jobs
 * table, minus the dW3 jobs that row jobs replace (HINT_DW3_ROWS: units with at most 4 outputs), followed by those row jobs.
 * j = -1: field 0 the jobs of the list, 1 the single-tile jobs among them, 2 the row jobs at its end, 3 and 4 the jobs and the
 * single-tile jobs of the table itself.  j >= 0, one value of job j: [0] P operand (2 g_st, 8 rebuilt g2, 9 g_st of a row job, ..)
 * [1] its first column  [2] output rows M  [3] 16-row tiles of M  [4] Q operand (4 a2, ..)  [5] its first column  [6] output
 * columns N  [7] 16-column tiles of N (row jobs: 64-column quads)  [8] row stride of the output  [9] float offset of out[0][0] in the
 * flat gradient  [10] float offset of the bias gradient or -1  [11] [12] [13] [14] the unit's outputs r, its first g_st column, its
 * hidden width, its first a2 column.  INT64_MIN on error (hint_last_error). */
#define HINT_WJOB_FIELDS 15
int64_t hint_plan_check_wjob(const hint_node_desc* nodes, int32_t n_nodes, int32_t d, int32_t dc, float clamp, int32_t variant,
                             int64_t j, int32_t field);

/* Re-pack the flat parameters into `packed` (hint_plan_packed_floats floats).  Must be called
 * after every change of the parameters and before the next forward / inverse / backward that
 * should see it; one small launch (the weights of a block are a few hundred KiB). */
int hint_block_pack(const hint_plan* plan, const float* params, float* packed, void* stream);

/* The same for several blocks in ONE launch (a trainer re-packs every block of the flow after
 * each optimizer step): the group records plan / params / packed pointers of n blocks once. */
typedef struct hint_pack_group hint_pack_group;
int hint_pack_group_create(const hint_plan* const* plans, const float* const* params,
                           float* const* packed, int32_t n, hint_pack_group** out);
int hint_pack_group_run(const hint_pack_group* group, void* stream);
/* The same launch as the prologue of a training step: additionally clears zero_floats floats at
 * zero_buf (the loss sums of the step before; NULL/0 = nothing), adds 1 to rng_state[1] (the step
 * counter t of hint_chain_forward_noisy; NULL = no counter) and, if opt_state is given (device
 * float[5] = {lr, beta1, beta2, out, out}; needs rng_state), writes Adam's factors of step t,
 * opt_state[3] = lr / (1 - beta1^t) and opt_state[4] = 1 / sqrt(1 - beta2^t), for
 * hint_adam_step_dev. */
int hint_pack_group_run_ex(const hint_pack_group* group, float* zero_buf, int32_t zero_floats,
                           uint64_t* rng_state, float* opt_state, void* stream);
void hint_pack_group_destroy(hint_pack_group* group);

/* z, J = block(x | c), rev=False (hint.py:62-80,90,97-99).  c may be NULL iff dc == 0.
 * params: flat parameters (biases are read from here); packed: output of hint_block_pack.
 * tape: NULL for inference, else hint_plan_tape_floats(plan, B) floats (training).
 * Non-finite data (every forward / inverse entry point, block and chain): a row with a NaN or inf in x or c changes no bit of
 * any other row, and its objective 0.5 |z|^2 - J (the inverse's x row) is non-finite where the reference's is; which lanes,
 * and whether J alone, are non-finite is not specified. */
int hint_block_forward(const hint_plan* plan, const float* params, const float* packed,
                       const float* x, const float* c, float* z, float* J, float* tape, int32_t B,
                       void* stream);
/* x, J = block(z | c), rev=True: own coupling undone first, then children
 * (hint.py:82-88); J is the NEGATED log-det like the reference returns it (hint.py:83). */
int hint_block_inverse(const hint_plan* plan, const float* params, const float* packed,
                       const float* z, const float* c, float* x, float* J, int32_t B, void* stream);
/* Backward of hint_block_forward.  Takes the block INPUT x and the tape the forward call
 * recorded (required), upstream g_z [B,d] and
 * g_J [B] (either may be NULL = zeros).  Writes g_x [B,d], g_c [B,dc] (may be NULL) and the
 * flat parameter gradient g_params (same layout as params): overwritten when accumulate == 0,
 * added to when accumulate != 0 (the caller then owns zeroing, e.g. hint_adam_step's
 * zero_grads); 16-byte aligned.  Every gradient is reduced in a fixed order (per-split slabs, then one
 * reduction pass; no float atomics): the same inputs give bit-identical gradients.  workspace:
 * hint_plan_workspace_bytes(plan, B) bytes, 16-byte aligned device scratch. */
int hint_block_backward(const hint_plan* plan, const float* params, const float* packed,
                        const float* x, const float* tape, const float* c, const float* g_z,
                        const float* g_J, float* g_x, float* g_c, float* g_params,
                        int32_t accumulate, void* workspace, size_t workspace_bytes, int32_t B,
                        void* stream);

/* Backward of hint_block_inverse / hint_block_inverse_ex: what autograd derives when `rev=True` runs with gradients
 * (hint.py:82-88 and the recursion of :85-88 are differentiable torch ops; train_unconditional.py:152-153 only samples
 * under no_grad, so no reference loop needs it - it is here for users of the module who do).
 *   x        [B,d] the OUTPUT of the inverse call (with the same perm, if any); c as given to it.
 *   g_x, g_J upstream gradients of the inverse's outputs (either may be NULL = zeros).
 *   g_z [B,d], g_c [B,dc] (may be NULL), g_params (flat, same layout as params; overwritten when accumulate == 0, added
 *   to otherwise; 16-byte aligned) receive the gradients.
 *   perm     the matrix given to hint_block_inverse_ex (x = block^-1(z) @ perm^T), or NULL.
 * Runs level by level on the block kernels, deepest level first: the forward direction rebuilds from x what the
 * inverse saw at every node, and each level's derivative is the forward coupling's with the roles turned round
 * (g_z2 = g_x2 / e(s), all subnet gradients with the opposite sign; derivation: DESIGN.md section 1).  The first call
 * on a plan builds one plan per tree level (device tables; not stream-ordered, like hint_plan_create).
 * workspace: hint_plan_inverse_workspace_bytes(plan, B) bytes of 16-byte aligned device scratch (that call builds the
 * level plans as well; returns 0 on failure, see hint_last_error). */
size_t hint_plan_inverse_workspace_bytes(const hint_plan* plan, int32_t B);
int hint_block_inverse_backward(const hint_plan* plan, const float* params, const float* x, const float* c,
                                const float* g_x, const float* g_J, float* g_z, float* g_c, float* g_params,
                                int32_t accumulate, void* workspace, size_t workspace_bytes, const float* perm,
                                int32_t B, void* stream);

/* Chained forms used by the flow container / trainer (hint_amd/flow.py, hint_amd/train.py): the
 * work FrEIA's graph does between two blocks is folded into the block kernels.
 *   perm     [d,d] row-major fixed orthogonal matrix of the permutation node in front of the
 *            block (power_hint_8.py:59-62): forward computes block(x @ perm), inverse returns
 *            block^-1(z) @ perm^T, backward returns g_x @ perm^T.  NULL = none.  With perm the
 *            forward stores the permuted input in the last [B,d] slice of the tape and backward
 *            reads it from there (x may be NULL).
 *   J_in     [B] log-det accumulated by the preceding blocks, added to this block's J
 *            (ReversibleGraphNet.log_jacobian sums the nodes); NULL = 0.
 *   loss_acc float[64][2], accumulated atomically (workgroup b adds to slot b % 64, the caller
 *            sums the slots): [.][0] += sum_rows 0.5*|z|^2, [.][1] += sum_rows J (the two loss
 *            terms of train_unconditional.py:128-129 before the .mean()); NULL = skip.
 *   gz_scale multiplies g_z on load (pass z and 1/B for the first term's gradient);
 *   gJ_const used for every row when g_J is NULL (-1/B for the second term). */
int hint_block_forward_ex(const hint_plan* plan, const float* params, const float* packed,
                          const float* x, const float* c, float* z, float* J, float* tape,
                          const float* perm, const float* J_in, float* loss_acc, int32_t B,
                          void* stream);
int hint_block_inverse_ex(const hint_plan* plan, const float* params, const float* packed,
                          const float* z, const float* c, float* x, float* J, const float* perm,
                          const float* J_in, int32_t B, void* stream);
int hint_block_backward_ex(const hint_plan* plan, const float* params, const float* packed,
                           const float* x, const float* tape, const float* c, const float* g_z,
                           const float* g_J, float* g_x, float* g_c, float* g_params,
                           int32_t accumulate, void* workspace, size_t workspace_bytes,
                           const float* perm, float gz_scale, float gJ_const, int32_t B,
                           void* stream);

/* Whole-flow launches.  A chain is n_blocks blocks of ONE plan (the configs stack identical
 * blocks, power_hint_8.py:56-67), each with its own parameters, optional permutation in front,
 * tape and backward workspace, laid out for a fixed batch size B.  hint_chain_forward runs
 * all blocks in one kernel (the lane tile of a row stays on chip from block to block; what
 * ReversibleGraphNet.forward does node by node), hint_chain_backward runs the row-parallel
 * part of all blocks in one kernel and all weight gradients in a second one.
 *   hint_chain_set_block: pointers of block i; they are captured, not copied, and must stay
 *     valid.  tape: hint_plan_tape_floats(plan, B) floats (required for training).  workspace /
 *     g_params may be NULL for an inference-only chain.
 *   hint_chain_commit: uploads the table (synchronous); call after the last set_block and
 *     before the first forward/backward (and again after changing a block).
 *   forward: z [B,d], J [B] = sum of the blocks' log-dets (+ J_in); loss_acc as in
 *     hint_block_forward_ex.  x may alias z.
 *   backward: arguments as in hint_block_backward_ex; x is only read when block 0 has no
 *     permutation.  g_c accumulates over the blocks (all blocks see the same c). */
typedef struct hint_chain hint_chain;
int hint_chain_create(const hint_plan* plan, int32_t n_blocks, int32_t B, hint_chain** out);
int hint_chain_set_block(hint_chain* chain, int32_t i, const float* params, const float* packed,
                         const float* perm, float* tape, void* workspace, size_t workspace_bytes,
                         float* g_params);
int hint_chain_commit(hint_chain* chain);
int hint_chain_forward(const hint_chain* chain, const float* x, const float* c, float* z, float* J,
                       const float* J_in, float* loss_acc, void* stream);
/* hint_chain_forward on x + noise * N(0,1) (train_unconditional.py:121), the noise drawn inside
 * the kernel: Philox4x32-10 keyed by rng_state = {seed, step} (device memory, read only here;
 * hint_pack_group_run_ex advances step) and the element index, Box-Muller.  x_noisy [B,d]
 * (may be NULL) receives the perturbed input, which is what hint_chain_backward must be given
 * as x.  rng_state == NULL: no noise. */
int hint_chain_forward_noisy(const hint_chain* chain, const float* x, const float* c, float* z,
                             float* J, const float* J_in, float* loss_acc, float noise,
                             const uint64_t* rng_state, float* x_noisy, void* stream);
int hint_chain_backward(const hint_chain* chain, const float* x, const float* c, const float* g_z,
                        const float* g_J, float* g_x, float* g_c, float gz_scale, float gJ_const,
                        int32_t accumulate, void* stream);
/* The same with the two halves of the backward pass selectable per call (profiling, or overlapping
 * part B with other work): parts bit 0 = the row-parallel kernel (g_x, g_c and the per-row factors in
 * the workspace), bit 1 = the weight-gradient kernels (read what bit 0 left in the workspace). */
int hint_chain_backward_parts(const hint_chain* chain, const float* x, const float* c, const float* g_z,
                              const float* g_J, float* g_x, float* g_c, float gz_scale, float gJ_const,
                              int32_t accumulate, int32_t parts, void* stream);
/* Part B (the weight-gradient kernels) for the blocks [block_begin, block_end) of the chain only: a data-parallel
 * step finishes the gradient of the last blocks first and starts their all-reduce while the rest of part B runs
 * (one bucket per call; the blocks' gradients are whatever g_params slices hint_chain_set_block was given).  Part A
 * (hint_chain_backward_parts, parts = 1) must have run. */
int hint_chain_wgrad_range(const hint_chain* chain, const float* x, const float* c, int32_t accumulate,
                           int32_t block_begin, int32_t block_end, void* stream);
/* Sampling direction (train_unconditional.py:152-153, rev=True through the whole graph): the blocks
 * of the chain last to first in ONE launch, x = chain^-1(z), J = J_in - sum of the blocks' log-dets
 * (the reference's rev=True sign, hint.py:83).  x may alias z. */
int hint_chain_inverse(const hint_chain* chain, const float* z, const float* c, float* x, float* J,
                       const float* J_in, void* stream);
/* hint_chain_backward with the optimizer folded into the weight gradients' final reduction (one process: nothing sits
 * between backward and the step - train_unconditional.py:137-144): every parameter element takes its clamp + Adam step
 * (hint_adam_step_dev's arithmetic, bit for bit) the moment its gradient is summed, and the gradient arena is neither read
 * nor written.  params / exp_avg / exp_avg_sq: arenas of n floats that hold every block's parameter slice (the blocks'
 * params pointers must point into [params, params + n)); elements outside the blocks' slices are not touched. */
int hint_chain_backward_adam(const hint_chain* chain, const float* x, const float* c, const float* g_z, const float* g_J,
                             float* g_x, float* g_c, float gz_scale, float gJ_const, float* params, float* exp_avg,
                             float* exp_avg_sq, int64_t n, const float* opt_state, float beta1, float beta2, float eps,
                             float weight_decay, float grad_scale, float grad_clamp, void* stream);
void hint_chain_destroy(hint_chain* chain);

/* ---- modules that run as launches of their own and share ONE part B (round 5; abi 6) ----
 * The conditional two-lane model (configs/plus_shape/conditional_hint_4_full.py:58-94) is a graph, not a chain: its x lane's
 * blocks take the y lane as their condition, so every module's forward and row-parallel backward is a launch of its own.
 * Their weight gradients need not be: the modules of one plan are gathered in a chain whose blocks carry their OWN level-0
 * input (x_in: what the module's forward was given; NULL when it had a fused permutation - the tape holds the permuted input)
 * and condition (c_in), and hint_chain_wgrad_range / hint_chain_wgrad_adam run part B and its slab reduction for all of them
 * in one launch each.  A chain with such blocks serves part B only.  g_add (any chain): a [B, d] gradient the backward's part A
 * adds to block i's input gradient before it goes back through the block's fused permutation - the block's permuted input had
 * a second consumer (the y lane after its permutation is also the x lane's condition, train_conditional.py:50-55 graph).
 * Call between hint_chain_set_block(i) and hint_chain_commit. */
int hint_chain_set_block_io(hint_chain* chain, int32_t i, const float* x_in, const float* c_in, const float* g_add);
/* part B + slab reduction of every block of the chain with the clamp + Adam step in the reduction (hint_chain_backward_adam
 * without part A): the row-parallel launches (hint_block_backward_rows, hint_chain_backward_parts(.., parts = 1, ..)) have
 * left the per-row factors in the blocks' workspaces. */
int hint_chain_wgrad_adam(const hint_chain* chain, const float* x, const float* c, float* params, float* exp_avg,
                          float* exp_avg_sq, int64_t n, const float* opt_state, float beta1, float beta2, float eps,
                          float weight_decay, float grad_scale, float grad_clamp, void* stream);
/* hint_block_forward_ex with the dequantisation noise of train_conditional.py:121 drawn in the kernel (Philox4x32-10 keyed by
 * rng_state = {seed, step}; x_noisy [B,d] receives the perturbed input the backward pass starts from); noise = 0: plain. */
int hint_block_forward_noisy(const hint_plan* plan, const float* params, const float* packed, const float* x,
                             const float* c, float* z, float* J, float* tape, const float* perm,
                             const float* J_in, float* loss_acc, float noise, const uint64_t* rng_state,
                             float* x_noisy, int32_t B, void* stream);
/* the row-parallel part of hint_block_backward_ex alone: g_x, g_c, and the per-row factors of the weight gradients in
 * `workspace` (hint_plan_workspace_bytes) for a later part B over a chain that holds this block with that workspace. */
int hint_block_backward_rows(const hint_plan* plan, const float* params, const float* packed, const float* x,
                             const float* tape, const float* c, const float* g_z, const float* g_J, float* g_x,
                             float* g_c, void* workspace, size_t workspace_bytes, const float* perm, float gz_scale,
                             float gJ_const, int32_t B, void* stream);

/* ---- posterior sampling of the conditional model (abi 8, additive) ----
 * For one observation y the reference's ExternalAffineCoupling ac_y_to_x_i (configs/plus_shape/conditional_hint_4_full.py:76-82)
 * is a fixed per-lane affine map of the x lane: its s and t nets see the condition only.  model_inverse / sample_conditional
 * (conditional_hint_4_full.py:99-113, called by train_conditional.py:36-47 and timed by rejection_sampling.py:168-213) and the
 * x-lane density of evaluate(only_x=True) (train_conditional.py:58-100) then reduce to the coefficients of the four couplings
 * and ONE chained launch over the x lane's hierarchical blocks.
 *   hint_block_ext_coeffs: plan = a one-node plan whose upper half is empty (node k = 0, dc > 0: an ExternalAffineCoupling);
 *     params / packed as for hint_block_forward (packed must be current: hint_block_pack); c [R, dc] condition rows.  Writes
 *     coef_out [R][2][d] = (clamp * 0.636 * atan(s), t) per row (hint.py:56-60, the plan's clamp), what the coupling's forward
 *     applies as x' = x e^a + t, J += sum a.  No argument may be NULL; R = 0 does nothing.  A row of c that holds a NaN or an
 *     inf gets NaN coefficients (as the reference's subnets give it), and changes no other row.
 *   hint_chain_set_block_affine: block i of an INFERENCE chain (set without tape) gets an element-wise affine step behind its
 *     tree: forward x' = x exp(a) + b, J += sum a; hint_chain_inverse undoes it in front of the tree's inverse, J -= sum a.
 *     Row r of the batch reads a = coef + r * row_stride, b = a + d (row_stride = 0: one row of coefficients for every row of
 *     the batch; 2d: one per row, hint_block_ext_coeffs' layout).  coef NULL removes the step.  Call after
 *     hint_chain_set_block(i) (which clears it) and before hint_chain_commit; the pointer is captured, not copied.  Fails for a
 *     training chain (block set with a tape), and for a chain whose plan runs this B on the wave-local kernels (narrow trees:
 *     hint_plan_dispatch field 0), which have no affine step. */
int hint_block_ext_coeffs(const hint_plan* plan, const float* params, const float* packed, const float* c, int32_t R,
                          float* coef_out, void* stream);
int hint_chain_set_block_affine(hint_chain* chain, int32_t i, const float* coef, int64_t row_stride);

/* Fused gradient clamp + Adam step over a flat fp32 arena of n parameters; replaces
 *   for p in params: p.grad.data.clamp_(-5, 5)        (train_unconditional.py:140-141)
 *   torch.optim.Adam(..., eps, weight_decay).step()    (train_unconditional.py:144,174-176)
 * g' = clamp(grads*grad_scale, +-grad_clamp) + weight_decay*p, then the standard Adam update
 * with bias correction for the 1-based `step`.  grad_scale = 1/world_size turns the summed
 * all-reduce into the mean BEFORE the clamp; grad_clamp <= 0 disables clamping.  With
 * zero_grads != 0 the gradient arena is cleared after it has been consumed.  All four buffers
 * must be 16-byte aligned.
 * Non-finite gradients take the step those statements take: the clamp is torch.clamp's, so a NaN
 * gradient stays NaN (p, exp_avg and exp_avg_sq of that element become NaN and stay so) and +-inf
 * becomes +-grad_clamp; with grad_clamp <= 0 nothing is clamped at all, so an inf gradient makes both
 * moments inf and p NaN, as torch.optim.Adam alone does.  Every route that takes this step
 * (hint_adam_step_dev, hint_adam_multi_step, hint_chain_backward_adam, hint_chain_wgrad_adam) shares it. */
int hint_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                   int32_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                   float grad_scale, float grad_clamp, int32_t zero_grads, void* stream);
/* The same step with its step-dependent factors read from device memory (opt_state as written by
 * hint_pack_group_run_ex), so that the launch carries no per-step host argument and can be
 * captured in a graph together with the kernels of the step. */
int hint_adam_step_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                       const float* opt_state, float beta1, float beta2, float eps,
                       float weight_decay, float grad_scale, float grad_clamp, int32_t zero_grads,
                       void* stream);

/* The same clamp + Adam step for a model whose parameters live in MANY buffers (one arena per block, the twelve modules of
 * the conditional model, tensors of other modules): one launch over a table of segments, for a training loop that keeps its
 * own statements and only replaces
 *   for p in params_trainable: p.grad.data.clamp_(-5.00, 5.00)     (train_unconditional.py:140-141, train_conditional.py:146-147)
 *   optim.step()                                                     (train_unconditional.py:144, train_conditional.py:150;
 *                                                                     the torch.optim.Adam of :174-176 / :180-182)
 * A segment is n consecutive floats of parameters, gradients and both moments; every element takes the arithmetic of the
 * flat-arena step above, bit for bit.  Pointers need 4-byte alignment only: where the four pointers of a segment agree
 * modulo 16 the step moves 16 bytes per lane, elsewhere single floats.  n may be 0.  The p ranges of two segments must not
 * overlap.  The table is copied to device memory when the handle is created (synchronous; the current device); the buffers
 * themselves are read at each step only, and only p, g, m, v - nothing else needs initialising.
 *   multi_create   rejects (before any device call) a null pointer, a negative n, a misaligned pointer, overlapping p ranges;
 *                  n_segs == 0 gives a valid handle whose step does nothing.
 *   multi_step     step, lr, ..., zero_grads as in the flat-arena step; stream-ordered, no host-device traffic.
 *   multi_chunk    host only: how multi_create cuts the segments into the work items of the launch.  c == -1 returns their
 *                  number; 0 <= c < number returns field 0 (segment), 1 (first float) or 2 (floats) of chunk c; -1 on an error.
 *                  Every float of every segment is in exactly one chunk; a chunk has at most 1024 (+3 in front of a segment's
 *                  first 16-byte boundary) floats.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the table.  (out is host memory:
 * the handle.) */
typedef struct hint_adam_seg { float* p; float* g; float* m; float* v; int64_t n; } hint_adam_seg;
typedef struct hint_adam_multi hint_adam_multi;
typedef hint_adam_multi** hint_adam_multi_out;
int hint_adam_multi_create(const hint_adam_seg* segs, int32_t n_segs, hint_adam_multi_out out);
int hint_adam_multi_step(const hint_adam_multi* h, int32_t step, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float grad_scale, float grad_clamp, int32_t zero_grads, void* stream);
void hint_adam_multi_destroy(const hint_adam_multi* h);
int64_t hint_adam_multi_chunk(const hint_adam_seg* segs, int32_t n_segs, int64_t c, int32_t field);

/* Multi-kernel MMD, the sample-quality metric of the reference's evaluation loop (rejection_sampling.py:56-73 multi_mmd, called on
 * 4000 x 4000 pairs per model and run by compare_unconditional / compare_conditional).  For x [n_x, d], y [n_y, d] and kernels
 * (C_k, a_k), k < n_kernels:
 *   k(D) = sum_k C_k^a_k ((C_k + D) / a_k)^(-a_k),  D = max(|u - v|^2, 0)
 *   MMD  = mean_ij k(D(x_i, x_j)) + mean_ij k(D(y_i, y_j)) - 2 mean_ij k(D(x_i, y_j))
 * over all pairs, the diagonal included (the biased V-statistic; multi_mmd's value for n_x == n_y, each term's own mean otherwise).
 * out = {MMD, mean XX, mean YY, mean XY}; the MMD is formed from the three means as stored, so every float of out is written and
 * a run that is handed mean YY (yy: out[2] of an earlier run on the same y and kernels; no YY tile is computed then) returns the
 * same bits.  Both sets are centred on y's mean before the Gram products; D is exactly 0 for a row against itself.  The result
 * does not depend on what the workspace or out held, and two runs on the same inputs agree bit for bit (no atomics).
 *   run              stream-ordered on the current device: four launches, no host synchronisation, no allocation (capturable).
 *                    Rejects, before any device call and naming the field: a null x, y, out or workspace; n_x, n_y or d < 1;
 *                    d > 4096; n_x or n_y > 1048576; n_kernels outside 1..8; a width or exponent that is not positive and finite;
 *                    a pointer that is not 4-byte (workspace: 16-byte) aligned; a workspace smaller than workspace_bytes says.
 *   workspace_bytes  0 (and an error message) for sizes run would reject.
 *   job              host only: the work items of the pair launch, one T x T tile of a pair matrix each.  j == -1: field 0 is
 *                    their number, field 1 is T.  0 <= j < number: field 0 kind (0 XX, 1 YY, 2 XY), 1 tile row, 2 tile column,
 *                    3 weight (XX and YY run on tile columns >= tile rows only; off-diagonal tiles weigh 2).  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_mmd_desc {
    const float* x; const float* y;        /* [n_x, d], [n_y, d] row-major, 4-byte aligned */
    int32_t n_x, n_y, d, n_kernels;        /* n_kernels 1..8 */
    float width[8], exponent[8];           /* C_k > 0, a_k > 0 */
    const float* yy;                       /* NULL, or device float: mean YY of an earlier run on the same y and kernels */
    float* out;                            /* device float[4] */
    void* workspace; size_t workspace_bytes;
} hint_mmd_desc;
size_t hint_mmd_workspace_bytes(int32_t n_x, int32_t n_y, int32_t d);
int hint_mmd_run(const hint_mmd_desc* desc, void* stream);
int64_t hint_mmd_job(int32_t n_x, int32_t n_y, int32_t with_yy, int64_t j, int32_t field);

/* ABC selection, the ground-truth posterior sample of the reference's evaluation loop (rejection_sampling.py:88-96 quantile_ABC,
 * called at :188 by compare_conditional on 1e8 prior observations per run).  For y [n_rows, ny], a target t [ny] and k:
 *   D_i = sum_j (y_ij - t_j)^2 in fp32, j = 0, 1, .., ny - 1 in that order: the first term a rounded product, every later one a fused
 *         multiply-add onto the sum; a D_i that is not a finite number (inf, NaN) counts as +inf
 *   rows are totally ordered by (D_i, i); idx / dist = the first k rows of that order and sqrt(D) of each, ascending
 * The selection is exact (a radix select over the bit pattern of D, y re-read on every pass: field 2 of geometry passes, nothing of
 * size n_rows is stored), does not depend on what idx, dist or the workspace held, and two runs agree bit for bit (integer counts
 * only, no float atomics, no global counters).
 *   run              stream-ordered on the current device: no host synchronisation, no allocation (capturable).  Rejects, before
 *                    any device call and naming the field: a null y, target, idx, dist or workspace; n_rows outside 1..2^30; ny
 *                    outside 1..32; k outside 1..min(n_rows, 8192); a pointer that is not 4-byte (workspace: 16-byte) aligned; a
 *                    workspace smaller than workspace_bytes says.
 *   workspace_bytes  0 (and an error message) for sizes run would reject.  At most 8.5 MiB, whatever n_rows is.
 *   geometry         host only: field 0 the workgroups of the streaming passes, 1 the rows each owns (workgroup w: rows
 *                    [w rows, min(n_rows, (w + 1) rows))), 2 the passes over y.  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_abc_desc {
    const float* y;                        /* [n_rows, ny] row-major, 4-byte aligned */
    const float* target;                   /* device float[ny] */
    int64_t n_rows;
    int32_t ny, k;
    int32_t* idx;                          /* device int32[k] */
    float* dist;                           /* device float[k] */
    void* workspace; size_t workspace_bytes;
} hint_abc_desc;
size_t hint_abc_workspace_bytes(int64_t n_rows, int32_t ny, int32_t k);
int hint_abc_run(const hint_abc_desc* desc, void* stream);
int64_t hint_abc_geometry(int64_t n_rows, int32_t ny, int32_t field);

/* The lens-shape simulator and the target distance of the reference's evaluation loop (data.py:127-139 LensShapeModel.forward_process
 * over data.py:51-57 trace_fourier_curves, a Python loop with a 100 x 100 pdist matrix per row; rejection_sampling.py:99-102
 * mean_target_distance, called at :204 on 4000 samples per model and run; rejection_sampling.py:76-85 prepare_samples runs the
 * simulator over 1e8 prior rows).  For x [n_rows, 4 K], K = n_coeffs odd, laid out as data.py:30-40 flatten_coeffs does (x[:, :2K]
 * real parts as [2 axes, K], x[:, 2K:] imaginary parts; coefficient k belongs to frequency m = k - K/2), and P = n_points:
 *   p[t, axis] = sum_k re[axis,k] cos(2 pi m t / (P-1)) - im[axis,k] sin(2 pi m t / (P-1)), t = 0 .. P-1: fp32 fused multiply-adds
 *         onto the sum over k ascending (real term, then imaginary term); each twiddle the true value rounded to fp32, the angle
 *         reduced exactly ((|m| t) mod (P-1) in integers, sincospi in double), so point P-1 repeats point 0 bit for bit
 *   D(i,j) = fma(dy, dy, dx dx) of p_i - p_j in fp32, i < j; the chosen pair is the first maximum in row-major (i, j) order, a NaN
 *         D never wins, the start value is pair (0, 1)
 *   y[row] = (p_j.y - p_i.y, p_j.x - p_i.x), each fma(noise, eps[row], .) when eps is given
 *   dist[row] = sqrt(fma(d1, d1, d0 d0)), d = y[row] - target;  mean = (sum of dist in double) / n_rows as fp32, summed in a fixed
 *         order: per wavefront over its consecutive rows, then over the wavefronts in row order (no float atomics, no counters)
 * A row's y and dist do not depend on n_rows, on where the row stands, on max_groups or on what y, dist, mean or the workspace
 * held; two runs agree bit for bit.  Rows with non-finite x give unspecified values and disturb no other row.
 *   run              stream-ordered on the current device: one launch (two with mean), no host synchronisation, no allocation
 *                    (capturable).  eps, target, dist, mean may be NULL; the workspace is used (and checked) only with mean.
 *                    max_groups: 0 = the default grid, otherwise the workgroups at most (values above the cap mean the cap).
 *                    Rejects, before any device call and naming the field: a null x or y; n_rows outside 1..2^30; n_coeffs even
 *                    or outside 1..25; n_points outside 2..128; dist or mean without target; max_groups < 0; a noise that is not
 *                    finite; a pointer that is not 4-byte (workspace: 16-byte) aligned; with mean, a null workspace or one smaller
 *                    than workspace_bytes says.
 *   workspace_bytes  0 (and an error message) for sizes run would reject.  64 KiB whatever n_rows is (one double per wavefront
 *                    of the largest grid).
 *   geometry         host only, for the default grid: field 0 the workgroups, 1 the rows a workgroup has in flight (a tile: one per
 *                    wavefront), 2 the consecutive rows each wavefront owns (wavefront q: rows [q R, min(n_rows, (q + 1) R)),
 *                    R = ceil(n_rows / (tile x workgroups))), 3 the grid cap.  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_curve_desc {
    const float* x;                        /* [n_rows, 4 n_coeffs] row-major, 4-byte aligned */
    int64_t n_rows;
    int32_t n_coeffs, n_points;            /* K odd 1..25, P 2..128 */
    const float* eps;                      /* NULL, or device float[n_rows, 2] */
    float noise;
    const float* target;                   /* NULL, or device float[2] */
    float* y;                              /* device float[n_rows, 2] */
    float* dist;                           /* NULL, or device float[n_rows] */
    float* mean;                           /* NULL, or device float */
    void* workspace; size_t workspace_bytes;
    int32_t max_groups;
} hint_curve_desc;
size_t hint_curve_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points);
int hint_curve_run(const hint_curve_desc* desc, void* stream);
int64_t hint_curve_geometry(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int32_t field);

/* Dense curve tracing and the distances of a curve to a template: the shape-quality columns of the reference's evaluation
 * (run_experiments.py:147-159 and eval_shapes.py:82-95 trace every sample with data.py:51-57 trace_fourier_curves at 100 and at 1000
 * points and call best_shape_fit.py:143-149 max_and_avg_hausdorff_distance per row, a [P, M, 2] numpy tensor each; the template is
 * best_shape_fit.py:195-199 lens_points_from_params, reached through :275-277, or the densified plus outline of :153-156;
 * best_shape_fit.py:203-209 points_to_lens_loss is the same two-sided minimum over squared distances).  Per row n of n_rows two
 * point sets are compared.
 *   B, the curve, P = n_points points, from exactly one source:
 *     traced  x [n_rows, 4 K] as hint_curve_desc's x: p[t, axis] by hint_curve_run's own rule - fp32 fused multiply-adds onto the
 *             sum over k ascending (real term, then imaginary term), each twiddle the true value rounded to fp32 after the exact
 *             reduction r = (|m| t) mod (P - 1) in integers (sincospi in double), so point P - 1 repeats point 0 bit for bit.  For
 *             P <= 128 the points are the bits hint_curve_run computes internally.
 *     given   b_points [n_rows, P, 2]: curves the caller traced already.
 *   A, the template, M_n points, 1 <= M_n <= 4096, taken from a_points [n_template, 2]: with a_offsets (int64 [n_rows + 1],
 *     ascending from 0 to n_template) row n owns a_points[a_offsets[n] : a_offsets[n + 1]] (ragged); without, every row shares all
 *     n_template points.  a_params [n_rows, 4] = (x, y, scale, angle), if given, applies lens_points_from_params - prototype times
 *     [[cos, sin], [-sin, cos]] (row vectors), times scale, plus (x, y) - in this order: cs, sn = sincos in double of the fp32 angle,
 *     rounded to fp32; qx = fma(-a.y, sn, a.x cs), qy = fma(a.y, cs, a.x sn); A = (fma(qx, scale, x), fma(qy, scale, y)).
 *     Without a_params the template is used as given.
 *   D(i, j) = fma(dy, dy, dx dx) of A_i - B_j in fp32;  mA_i = min_j D(i, j), mB_j = min_i D(i, j): exact functions of the points,
 *     whatever the order the minima are taken in.
 *   max_h [n_rows]      sqrt, correctly rounded, of the largest of all M_n + P minima
 *   avg_h [n_rows]      ((sum of the fp32 values sqrt(mA_i)) + (sum of sqrt(mB_j))) / (M_n + P), the sums and the division in
 *                       double, the result rounded to fp32
 *   chamfer [n_rows, 2] (sum_j mB_j / P, sum_i mA_i / M_n) the same way; points_to_lens_loss(prototype, points, params, w) is
 *                       chamfer[:, 0] + w chamfer[:, 1]
 *   points [n_rows, P, 2]  the traced curve (traced source only).  When points is the only output, neither the template nor
 *                       a_offsets nor a_params is read (a_points must still be non-NULL).
 *   The association of each of the four sums is fixed: lane l of wavefront v = thread 64 v + l first adds the values of its own
 *   points i = 256 c + 64 v + l (c ascending) to 0; the 64 lanes of a wavefront are added by a butterfly (lane distances 32, 16,
 *   8, 4, 2, 1); the four wavefronts are added in order.  No float atomics, no counters.
 * A row's outputs do not depend on n_rows, on where the row stands, on max_groups or on what the outputs held; two runs agree bit
 * for bit.  Rows with non-finite inputs give unspecified values, fault nothing and disturb no other row.  A ragged row whose range
 * is not 1..4096 points inside a_points (the offsets are on the device, so the host cannot check them) gets NaN in max_h, avg_h
 * and chamfer, and nothing outside a_points is read; its points, which do not depend on the template, are traced as usual.
 *   run              stream-ordered on the current device: one launch, no host synchronisation, no allocation (capturable).  Each
 *                    output may be NULL, not all four.  max_groups: 0 = the default grid, otherwise the workgroups at most.
 *                    Rejects, before any device call and naming the field: a null a_points; both or neither of x and b_points;
 *                    points with b_points; no output; n_rows outside 1..2^30; with x, n_coeffs even or outside 1..25 (ignored
 *                    with b_points); n_points outside 2..1024; n_template < 1; a shared template of more than 4096 points, ragged
 *                    ones of more than 4096 n_rows in all; max_groups < 0; a pointer that is not 4-byte (a_offsets: 8-byte) aligned.
 *   workspace_bytes  0: no workspace is needed, so the descriptor names none.  For sizes run would reject (n_coeffs = 0 stands
 *                    for the given source; max_template_points is the largest M_n) hint_last_error() says why, otherwise it is
 *                    left empty.
 *   geometry         host only, for the default grid: field 0 the workgroups, 1 the rows a workgroup has in flight (one), 2 the
 *                    template points of an LDS tile, 3 the grid cap, 4 the tiles of max_template_points.  Workgroup w of G takes
 *                    rows w, w + G, ...  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_hausdorff_desc {
    const float* x;                        /* NULL, or [n_rows, 4 n_coeffs] row-major: the traced source */
    const float* b_points;                 /* NULL, or device float[n_rows, n_points, 2]: the given source */
    int64_t n_rows;
    int32_t n_coeffs, n_points;            /* K odd 1..25 (traced source), P 2..1024 */
    const float* a_points;                 /* device float[n_template, 2] */
    const int64_t* a_offsets;              /* NULL (shared template), or device int64[n_rows + 1], 8-byte aligned */
    const float* a_params;                 /* NULL, or device float[n_rows, 4]: x, y, scale, angle */
    int64_t n_template;                    /* T: points in a_points */
    float* max_h;                          /* NULL, or device float[n_rows] */
    float* avg_h;                          /* NULL, or device float[n_rows] */
    float* chamfer;                        /* NULL, or device float[n_rows, 2] */
    float* points;                         /* NULL, or device float[n_rows, n_points, 2] */
    int32_t max_groups;
} hint_hausdorff_desc;
size_t hint_hausdorff_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t max_template_points);
int hint_hausdorff_run(const hint_hausdorff_desc* desc, void* stream);
int64_t hint_hausdorff_geometry(int64_t n_rows, int32_t n_points, int64_t max_template_points, int32_t field);

/* The plus shape's fit loss and its Hausdorff distances to a curve: the plus columns of the reference's shape evaluation
 * (eval_shapes.py:82-95 calls, per row, best_shape_fit.py:54-65 points_to_plus_loss - over best_shape_fit.py:26-50
 * plus_segments_from_params and best_shape_fit.py:15-22 squared_dists_points_to_line_segment - and best_shape_fit.py:153-156
 * max_and_avg_hausdorff_distance_plus_shape, whose template is data.py:176-186 densify_polyline of the outline).  Per row n the 9
 * fitted parameters params[n] = (xlength, ylength, xwidth, ywidth, xshift, yshift, xoffset, yoffset, angle) give the 12 outline
 * segments, the two terms of the fit loss and the distances of the curve B (as hint_hausdorff_desc's: traced from x [n_rows, 4 K]
 * by the same rule and the same bits, or given as b_points [n_rows, P, 2]) to the densified outline A, whose points are generated
 * inside the kernel and exist nowhere in memory.  All arithmetic is fp32, each operation rounded once, unless said otherwise.
 *   1. local vertices.  h(v) = 0.5 v (exact);  xleft = xshift - h(xlength), xright = xshift + h(xlength), xtop = h(xwidth),
 *      xbottom = -xtop, yright = h(ywidth), yleft = -yright, ybottom = yshift - h(ylength), ytop = yshift + h(ylength); then, with
 *      c = 0.01f and each clamp taken from the unclamped partner, xleft = min(xleft, yleft - c), xright = max(xright, yright + c),
 *      ytop = max(ytop, xtop + c), ybottom = min(ybottom, xbottom - c).  V0..V11 = (xleft, xtop), (yleft, xtop), (yleft, ytop),
 *      (yright, ytop), (yright, xtop), (xright, xtop), (xright, xbottom), (yright, xbottom), (yright, ybottom), (yleft, ybottom),
 *      (yleft, xbottom), (xleft, xbottom); segment s is (V_s, V_(s+1) mod 12).
 *   2. keep.  Segment s is kept iff its two local vertices differ (an exact comparison: local segments are axis-parallel; the
 *      reference filters before it rotates).  Bit s of keep[n] says so.  Only a zero width drops segments.
 *   3. placement, the lens rule with scale 1: cs, sn = sincos in double of the fp32 angle, rounded to fp32; qx = fma(-v.y, sn,
 *      v.x cs), qy = fma(v.y, cs, v.x sn); W = (qx + xoffset, qy + yoffset).  segments[n, s] = (W_s, W_(s+1)), kept or not.
 *   4. segment term.  For a kept segment (a, b) = (W_s, W_(s+1)) and a curve point p: n = b - a; L = sqrt(fma(n.y, n.y, n.x n.x));
 *      n = n / L; ap = a - p; len = max(0, min(L, -fma(ap.y, n.y, ap.x n.x))); v = (fma(len, n.x, ap.x), fma(len, n.y, ap.y));
 *      d2 = fma(v.y, v.y, v.x v.x).  loss[n, 0] = the mean over the P points of min over the kept s of d2.
 *   5. corner term.  loss[n, 1] = the mean over the kept segments' first vertices W_s of min_j fma(dy, dy, dx dx), (dx, dy) =
 *      W_s - B_j: the squared distance itself (the reference roots and squares again).  points_to_plus_loss(points, params, w) is
 *      loss[:, 0] + w loss[:, 1].
 *   6. densified outline.  The polygon is the kept segments' first vertices, in order, closed; the edge of kept segment s runs from
 *      E = W_s to S = the next kept first vertex, which is W_(s+1) bit for bit (a dropped segment's two vertices are the same
 *      bits).  count = max(1, rint(max(|S.x - E.x|, |S.y - E.y|) / max_dist)) in double from the fp32 vertices and the fp32
 *      max_dist, rint = round half to even.  Point i of count: E when count = 1; otherwise t = float(i) / float(count - 1), the
 *      correctly rounded quotient, and A = fma(t, S, (1 - t) E) per axis - both end points exact, so each vertex appears twice, as
 *      in the reference.  counts[n, s] = count, 0 for a dropped segment; M_n = their sum.
 *   7. distances.  D(i, j), mA_i, mB_j, max_h [n_rows] and avg_h [n_rows] between A (M_n points) and B (P points) exactly as
 *      hint_hausdorff_desc states them: the roots correctly rounded in fp32, their sums and the division by M_n + P in double.
 *      The association of every double sum is hint_hausdorff_run's: thread 64 v + l over its own points i = 256 c + 64 v + l (c
 *      ascending; for A, tile after tile of 1024 outline points), a butterfly over the lanes (distances 32 .. 1), the four
 *      wavefronts in order.  The segment term's sum over the P minima is added the same way and divided by P in double; the corner
 *      term's minima (exact, whatever the order) are added in double over s ascending and divided by the kept count.
 *   8. rows that cannot be served: M_n > 4096, a parameter that is not finite, a placed vertex or a quotient that is not finite.
 *      The quotient is cut at 8192 in double before it becomes an integer, so no loop bound comes from a wild value.  Such a row
 *      gets NaN in max_h and avg_h and counts[n, :] = -1; its segments, keep and loss need no outline and are computed as usual
 *      (unspecified for non-finite inputs).  Nothing faults and no other row is disturbed.
 *   9. A row's outputs do not depend on n_rows, on where the row stands, on max_groups or on what the outputs held; two runs agree
 *      bit for bit.  No float atomics, no counters.
 *   run              stream-ordered on the current device: one launch, no host synchronisation, no allocation (capturable).  Each
 *                    output may be NULL, not all six.  When none of loss, max_h and avg_h is asked, the curve is not read: x and
 *                    b_points may then both be NULL, and n_coeffs and n_points are looked at only if one of them is named.
 *                    max_groups: 0 = the default grid, otherwise the workgroups at most.  Rejects, before any device call and
 *                    naming the field: a null params; both of x and b_points; neither when loss, max_h or avg_h is asked; no
 *                    output; n_rows outside 1..2^30; with x, n_coeffs even or outside 1..25 (ignored with b_points); n_points
 *                    outside 2..1024; max_dist not finite or <= 0; max_groups < 0; a pointer that is not 4-byte aligned.
 *   workspace_bytes  0: no workspace is needed, so the descriptor names none.  For sizes run would reject (n_coeffs = 0 stands
 *                    for the given source) hint_last_error() says why, otherwise it is left empty.
 *   geometry         host only, for the default grid: field 0 the workgroups, 1 the rows a workgroup has in flight (one), 2 the
 *                    outline points of an LDS tile, 3 the grid cap, 4 the most outline points a row may have.  Workgroup w of G
 *                    takes rows w, w + G, ...  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_plus_desc {
    const float* x;                        /* NULL, or [n_rows, 4 n_coeffs] row-major: the traced source */
    const float* b_points;                 /* NULL, or device float[n_rows, n_points, 2]: the given source */
    int64_t n_rows;
    int32_t n_coeffs, n_points;            /* K odd 1..25 (traced source), P 2..1024 */
    const float* params;                   /* device float[n_rows, 9] */
    float max_dist;                        /* finite, > 0; the reference's value is 0.02 */
    int32_t max_groups;
    float* segments;                       /* NULL, or device float[n_rows, 12, 2, 2] */
    int32_t* keep;                         /* NULL, or device int32[n_rows]: bit s = segment s is kept */
    int32_t* counts;                       /* NULL, or device int32[n_rows, 12] */
    float* loss;                           /* NULL, or device float[n_rows, 2]: segment term, corner term */
    float* max_h;                          /* NULL, or device float[n_rows] */
    float* avg_h;                          /* NULL, or device float[n_rows] */
} hint_plus_desc;
size_t hint_plus_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points);
int hint_plus_run(const hint_plus_desc* desc, void* stream);
int64_t hint_plus_geometry(int64_t n_rows, int32_t n_points, int32_t field);

/* The lens-shape fit of a curve: the fit loss, its gradient and the whole SGD loop of the reference's fit in one launch
 * (run_experiments.py:150-159 calls, per row, best_shape_fit.py:230-261 fit_lens_shape_to_points: two starts of 100 autograd steps
 * of torch's SGD on best_shape_fit.py:203-209 points_to_lens_loss over best_shape_fit.py:195-199 lens_points_from_params).  Per row
 * n and start s the parameters p = (x, y, scale, angle) begin at starts[n, s] and take n_steps steps; the curve B (as
 * hint_hausdorff_desc's: traced from x [n_rows, 4 K] by the same rule and the same bits, or given as b_points [n_rows, P, 2]) is
 * compared with the prototype a_points [M, 2], 1 <= M <= 1024, shared by all rows (no ragged form).  All arithmetic is fp32, each
 * operation rounded once, unless said otherwise.
 *   1. evaluation at p.  The prototype is placed as hint_hausdorff_run places its template: cs, sn = sincos in double of the fp32
 *      angle, rounded to fp32; q = (fma(-a.y, sn, a.x cs), fma(a.y, cs, a.x sn)); A = (fma(q.x, scale, x), fma(q.y, scale, y)).
 *      e = A_i - B_j, D(i, j) = fma(e.y, e.y, e.x e.x).  mA_i = min_j D, taken at the lowest j among equal D; mB_j = min_i D, taken
 *      at the lowest i.  (The duplicate B_(P-1) = B_0 of a traced curve is therefore always resolved to j = 0, and both points
 *      count in the other direction, as in the reference.)  A NaN D is never selected; where nothing is, index 0 is.
 *   2. loss.  L = sum_j mB_j / P + w (sum_i mA_i / M): the sums and the divisions in double, in the association of
 *      hint_hausdorff_run's sums (thread 64 v + l over its own points 256 c + 64 v + l, c ascending; a butterfly over the lanes,
 *      distances 32 .. 1; the four wavefronts in order); L is rounded to fp32.  w = weight.
 *   3. gradient.  Each selected pair gives, from the recomputed e and q, the fp32 terms (e.x, e.y, fma(e.y, q.y, e.x q.x),
 *      fma(e.y, q.x, -(e.x q.y))).  Each term is added in double, in the same association, over the P pairs of B (sums SB) and
 *      over the M pairs of A (sums SA); then, in double, g = 2 (SB / P + w (SA / M)) for x, y and scale and scale times that for
 *      the angle; g is rounded to fp32.  This is the autograd gradient of points_to_lens_loss wherever the minima are unique.
 *   4. step i = 0 .. n_steps - 1 (torch's SGD with momentum and dampening 0 under StepLR with step_size 1): evaluate (L_i, g_i) at
 *      p_i; buf = g_0 at i = 0, else fma(momentum rounded to fp32, buf, g_i); p_(i+1) = fma(-lr_i, buf, p_i), where lr_i is the
 *      fp32 rounding of a double that starts at lr (at angle_lr for the angle) and is multiplied by gamma after every step.  The
 *      buffer and the rates start afresh for every start and every row.
 *   5. a start's result: all_params[n, s] = p_(n_steps); all_loss[n, s] = L_(n_steps - 1), the loss of the last step before its
 *      update, as the reference records it; grad[n, s] = g_(n_steps - 1).  n_steps = 0 is the evaluation alone: all_loss = L(p_0),
 *      grad = g(p_0), all_params = p_0.
 *   6. a row's result: the start with the smallest loss, the first one on a tie, gives params[n], loss[n] and best[n] (int32).  A
 *      NaN compares as larger; if every start's loss is NaN, start 0 is taken.
 *   7. trace[n, s, i] = (p_i [4], L_i, g_i [4]), 9 floats a step (n_steps >= 1).
 *   8. A row's outputs do not depend on n_rows, on where the row stands, on max_groups or on what the outputs held; two runs agree
 *      bit for bit.  No float atomics, no counters.
 *   9. A row with non-finite input gives unspecified values, faults nothing and disturbs no other row: every loop bound and every
 *      index range comes from the descriptor, never from data.
 *   run              stream-ordered on the current device: one launch, no workspace, no host synchronisation, no allocation
 *                    (capturable).  Each output may be NULL, not all seven.  max_groups: 0 = the default grid, otherwise the
 *                    workgroups at most.  Rejects, before any device call and naming the field: a null a_points or starts; both or
 *                    neither of x and b_points; no output; n_rows outside 1..2^30; with x, n_coeffs even or outside 1..25 (ignored
 *                    with b_points); n_points outside 2..1024; n_template outside 1..1024; n_starts outside 1..16; n_steps outside
 *                    0..1024; trace with n_steps = 0; lr, angle_lr, gamma or momentum not finite or negative; weight not finite;
 *                    max_groups < 0; a pointer that is not 4-byte aligned.
 *   workspace_bytes  0: no workspace is needed, so the descriptor names none.  For sizes run would reject (n_coeffs = 0 stands
 *                    for the given source) hint_last_error() says why, otherwise it is left empty.
 *   geometry         host only, for the default grid: field 0 the workgroups, 1 the rows a workgroup has in flight (one), 2 the
 *                    prototype points of an LDS tile, 3 the grid cap, 4 the most prototype points.  Workgroup w of G takes rows
 *                    w, w + G, ... and runs a row's starts one after the other.  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_lensfit_desc {
    const float* x;                        /* NULL, or [n_rows, 4 n_coeffs] row-major: the traced source */
    const float* b_points;                 /* NULL, or device float[n_rows, n_points, 2]: the given source */
    int64_t n_rows;
    int32_t n_coeffs, n_points;            /* K odd 1..25 (traced source), P 2..1024 */
    const float* a_points;                 /* device float[n_template, 2]: the prototype */
    int64_t n_template;                    /* M: 1..1024 */
    const float* starts;                   /* device float[n_rows, n_starts, 4]: x, y, scale, angle */
    int32_t n_starts, n_steps;             /* S 1..16; 0..1024 */
    double lr, angle_lr, gamma, momentum, weight;
    float* params;                         /* NULL, or device float[n_rows, 4] */
    float* loss;                           /* NULL, or device float[n_rows] */
    int32_t* best;                         /* NULL, or device int32[n_rows] */
    float* all_params;                     /* NULL, or device float[n_rows, n_starts, 4] */
    float* all_loss;                       /* NULL, or device float[n_rows, n_starts] */
    float* grad;                           /* NULL, or device float[n_rows, n_starts, 4] */
    float* trace;                          /* NULL, or device float[n_rows, n_starts, n_steps, 9] */
    int32_t max_groups;
} hint_lensfit_desc;
size_t hint_lensfit_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t n_template, int32_t n_starts,
                                    int32_t n_steps);
int hint_lensfit_run(const hint_lensfit_desc* desc, void* stream);
int64_t hint_lensfit_geometry(int64_t n_rows, int32_t n_points, int32_t field);

/* The plus-shape fit of a curve: the fit loss, its gradient by the nine parameters and the whole SGD loop of the reference's fit in
 * one launch (eval_shapes.py:85-87 calls, per row, best_shape_fit.py:93-129 fit_plus_shape_to_points: up to nine starts of 400
 * autograd steps of torch's SGD, best_shape_fit.py:108-118, on best_shape_fit.py:54-65 points_to_plus_loss with the corner weight of
 * :115, the early stop of :123-124 and the selection of :129).  Per row n and start s the parameters p = (xlength, ylength, xwidth,
 * ywidth, xshift, yshift, xoffset, yoffset, angle) begin at starts[n, s] and take n_steps steps; the curve B is hint_plus_desc's
 * (traced from x [n_rows, 4 K] by the same rule and the same bits, or given as b_points [n_rows, P, 2]).  All arithmetic is fp32,
 * each operation rounded once, unless said otherwise.
 *   1. geometry at p: hint_plus_desc's items 1 - 3, the same operations and the same bits - the local vertices and their clamps,
 *      the keep bits, the placed vertices W_0..W_11, and per kept segment s = (W_s, W_(s+1) mod 12) the constants a, n, L of its
 *      item 4.  nk = the kept segments; a dropped (zero-length) segment takes part in nothing below.
 *   2. segment term.  Per curve point p_j and kept segment s, in the order s = 0..11: ap, len, v and d2 as hint_plus_desc's item 4.
 *      The point's segment is the first s with the smallest d2 (a d2 replaces the minimum only when strictly smaller; a NaN never
 *      does; where nothing does, segment 0 with len = 0, v = 0).  With that segment's len and v: t = len / L (one fp32 division),
 *      and the four fp32 products v.x (1 - t), v.y (1 - t) (1 - t rounded first) for vertex s and v.x t, v.y t for vertex s + 1
 *      (mod 12).  |v|^2 has the derivative 2 v (1 - t) by W_s and 2 v t by W_(s+1) in all three cases of the clamp of len.
 *   3. corner term.  Per kept s: D_j = fma(dy, dy, dx dx), (dx, dy) = W_s - B_j; the corner's point j* is the one with the smallest
 *      D, the lowest j among equal D (a NaN D loses against every number).  Its derivative by W_s is 2 (W_s - B_j*), the fp32
 *      difference recomputed.
 *   4. sums, in double.  SEG = the sum over the P points of their minimum d2, in the association of hint_hausdorff_run's sums:
 *      thread 64 v + l over its own points 256 c + 64 v + l, c ascending; a butterfly over the lanes, distances 32 .. 1; the four
 *      wavefronts in order.  G_k [2] = for vertex k and either axis the sum of the products of item 2 that name the vertex, each
 *      point adding at most one of them: eight partial sums, partial j over the points j, j + 8, j + 16, ... in ascending order,
 *      then a butterfly over the eight (distances 4, 2, 1).  COR = the sum of the kept corners' minima over s ascending.
 *   5. loss and gradient, in double, c = the corner weight of the evaluation: L = SEG / P + c (COR / nk), rounded once to fp32.
 *      gW_k = (2 / P) G_k + [k kept] (2 c / nk) (W_k - B_j*).  With cs, sn the fp32 values of item 1 and V_k the local vertex:
 *      q_k = V_k R, R = [[cs, sn], [-sn, cs]] (row vectors); then over k ascending d xoffset = sum gW_k.x, d yoffset = sum
 *      gW_k.y, d angle = sum (gW_k.y q_k.x - gW_k.x q_k.y), and gV_k = gW_k R^T is added to the two of the eight clamped
 *      coordinates V_k is made of.  xtop, xbottom give +- 1/2 to d xwidth and yright, yleft +- 1/2 to d ywidth.  Each of the four
 *      clamped coordinates gives its derivative to the branch that was taken: unclamped, 1 to its shift and +- 1/2 to its length;
 *      clamped, +- 1/2 to the other bar's width.  When the two arguments of a clamp are equal the derivative goes to the
 *      unclamped side (torch's min / max split it equally there: a difference on a set of measure zero).  Each of the nine is
 *      rounded once to fp32.  This is the autograd gradient of points_to_plus_loss wherever the minima are unique.
 *   6. step i = 0 .. n_steps - 1 (torch's SGD with momentum and dampening 0 under StepLR with step_size 1): the corner weight is
 *      c_i = corner_weight (1 - i / n_steps) in double if corner_decay is not 0, else corner_weight; evaluate (L_i, g_i) at p_i;
 *      buf = g_0 at i = 0, else fma(momentum rounded to fp32, buf, g_i); p_(i+1) = fma(-lr_i, buf, p_i), where lr_i is the fp32
 *      rounding of a double that starts at lr (at angle_lr for the angle) and is multiplied by gamma after every step.  The buffer
 *      and the rates start afresh for every start and every row.
 *   7. a start's result: all_params[n, s] = p_(n_steps); all_loss[n, s] = L_(n_steps - 1), the loss of the last step before its
 *      update, as the reference records it; grad[n, s] = g_(n_steps - 1).  n_steps = 0 is one evaluation at corner_weight:
 *      all_loss = L(p_0), grad = g(p_0), all_params = p_0.  trace[n, s, i] = (p_i [9], L_i, g_i [9]), 19 floats a step.
 *   8. early stop: the starts run in order; when a start's loss (as a double) is < stop_loss, the row's remaining starts do not
 *      run.  A stop_loss that is <= 0 or NaN never stops, nor does a NaN loss.  n_run[n] (int32) = the starts that ran.  A start
 *      that did not run holds: all_params = the start itself, all_loss = +inf, grad and trace = quiet NaN (0x7fc00000) - every
 *      word of every requested output is written by every launch.
 *   9. a row's result: among the starts that ran the one with the smallest loss, the first one on a tie, gives params[n], loss[n]
 *      and best[n] (int32).  A NaN compares as larger; if every loss is NaN, start 0 is taken.
 *  10. A row's outputs do not depend on n_rows, on where the row stands, on max_groups or on what the outputs held; two runs agree
 *      bit for bit.  No float atomics, no counters.  A row with non-finite input gives unspecified values, faults nothing and
 *      disturbs no other row: every loop bound comes from the descriptor, and every index is a loop counter or a lane's number.
 *   run              stream-ordered on the current device: one launch, no workspace, no host synchronisation, no allocation
 *                    (capturable).  Each output may be NULL, not all eight.  max_groups: 0 = the default grid, otherwise the
 *                    workgroups at most.  Rejects, before any device call and naming the field: a null starts; both or neither of
 *                    x and b_points; no output; n_rows outside 1..2^30; with x, n_coeffs even or outside 1..25 (ignored with
 *                    b_points); n_points outside 2..1024; n_starts outside 1..16; n_steps outside 0..1024; trace with n_steps = 0;
 *                    lr, angle_lr, gamma or momentum not finite or negative; corner_weight not finite; max_groups < 0; a pointer
 *                    that is not 4-byte aligned.
 *   workspace_bytes  0: no workspace is needed, so the descriptor names none.  For sizes run would reject (n_coeffs = 0 stands
 *                    for the given source) hint_last_error() says why, otherwise it is left empty.
 *   geometry         host only, for the default grid: field 0 the workgroups, 1 the rows a workgroup has in flight (one), 2 the
 *                    curve points a thread holds at most, 3 the grid cap, 4 the most starts.  Workgroup w of G takes rows w,
 *                    w + G, ... and runs a row's starts one after the other.  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_plusfit_desc {
    const float* x;                        /* NULL, or [n_rows, 4 n_coeffs] row-major: the traced source */
    const float* b_points;                 /* NULL, or device float[n_rows, n_points, 2]: the given source */
    int64_t n_rows;
    int32_t n_coeffs, n_points;            /* K odd 1..25 (traced source), P 2..1024 */
    const float* starts;                   /* device float[n_rows, n_starts, 9] */
    int32_t n_starts, n_steps;             /* S 1..16; 0..1024 */
    double lr, angle_lr, gamma, momentum, corner_weight, stop_loss;
    int32_t corner_decay;                  /* not 0: the corner weight falls linearly to 0 over the steps */
    int32_t max_groups;
    float* params;                         /* NULL, or device float[n_rows, 9] */
    float* loss;                           /* NULL, or device float[n_rows] */
    int32_t* best;                         /* NULL, or device int32[n_rows] */
    int32_t* n_run;                        /* NULL, or device int32[n_rows] */
    float* all_params;                     /* NULL, or device float[n_rows, n_starts, 9] */
    float* all_loss;                       /* NULL, or device float[n_rows, n_starts] */
    float* grad;                           /* NULL, or device float[n_rows, n_starts, 9] */
    float* trace;                          /* NULL, or device float[n_rows, n_starts, n_steps, 19] */
} hint_plusfit_desc;
size_t hint_plusfit_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int32_t n_starts, int32_t n_steps);
int hint_plusfit_run(const hint_plusfit_desc* desc, void* stream);
int64_t hint_plusfit_geometry(int64_t n_rows, int32_t n_points, int32_t field);

/* IoU and DICE of a curve and a fitted shape: the first two columns of the reference's shape evaluation (run_experiments.py:144-167
 * and eval_shapes.py:82-103 call, per row, best_shape_fit.py:265-271 iou_and_dice_lens_shape or best_shape_fit.py:133-139
 * iou_and_dice_plus_shape: two shapely polygons, their intersection's and their union's area).  Per row n two closed polygons are
 * compared, with no clipping, no point-in-polygon test, no sorting and no topology.
 *   C, the curve, P = n_points vertices, 3 <= P <= 1024, from exactly one source, as hint_hausdorff_desc's B: traced from
 *     x [n_rows, 4 K] by the same rule and the same bits, or given as b_points [n_rows, P, 2].  Edge i runs from vertex i to vertex
 *     (i + 1) mod P; a traced curve's vertex P - 1 repeats vertex 0, so its edge P - 1 has no length.
 *   T, the template, M_n vertices, from exactly one source:
 *     a_points [n_template, 2], with a_offsets and a_params of hint_hausdorff_desc's meaning and placement (shared or ragged; cs, sn
 *       = sincos in double of the fp32 angle, rounded; q = (fma(-a.y, sn, a.x cs), fma(a.y, cs, a.x sn)); vertex = (fma(q.x, scale,
 *       x), fma(q.y, scale, y))), 3 <= M_n <= 4096;
 *     plus_params [n_rows, 9]: the twelve placed vertices W_0..W_11 of hint_plus_desc's items 1 and 3, the bits hint_plus_run
 *       writes to segments[n, s, 0]; M_n = 12.  All twelve are used: a dropped segment is an edge of no length.
 *   All arithmetic below is fp32, each operation rounded once, unless said otherwise.
 *   1. baseline.  y0 = the smallest y of all P + M_n vertices of the row (exact).  A vertex (x, y) is used as (x, h), h = y - y0
 *      >= 0.  An edge is (x0, h0, x1, h1) with dx = x1 - x0 and r = 1 / dx (a correctly rounded division).
 *   2. areas.  An edge's area term is (0.5 dx) (h0 + h1).  area_C = |the sum of the curve's P terms|, area_T = |the sum of the
 *      template's M_n terms|, the sums in double.
 *   3. the height of an edge at an abscissa q inside its x-range: u1 = min((q - x0) r, 1), u0 = min((x1 - q) r, 1),
 *      h = fma(u1, h1, u0 h0), then cut to the edge's own heights: max(min(h0, h1), min(max(h0, h1), h)).  Both weights are
 *      non-negative, so no slope, however steep, takes a height out of the edge's own range.
 *   4. the term of a curve edge e and a template edge f.  a = max(min(e.x0, e.x1), min(f.x0, f.x1)), b = min(max(e.x0, e.x1),
 *      max(f.x0, f.x1)); unless a < b the term is exactly 0 (so an edge with x1 = x0 contributes nothing).  w = b - a; ea, eb, fa,
 *      fb = the heights of e and f at a and at b; da = ea - fa, db = eb - fb; ma = min(ea, fa), mb = min(eb, fb).  When da and db
 *      have strictly opposite signs the heights cross inside: den = da - db, ta = da / den, tb = (-db) / den (two divisions),
 *      hc = fma(ta, eb, tb ea), sum = hc + fma(ta, ma, tb mb); otherwise sum = ma + mb.  term = (0.5 w) sum, negated when exactly
 *      one of e.x1 < e.x0 and f.x1 < f.x0 holds.  This is sign_e sign_f times the integral over [a, b] of the smaller height.
 *   5. I = |the sum of the P M_n terms| in double, then cut to [0, min(area_C, area_T)].  For simple polygons of either orientation
 *      this is the area of their intersection: the integral of the product of the two winding numbers.
 *   6. outputs, from the doubles: areas[n] = (area_T, area_C, I), iou[n] = I / (area_C + area_T - I), dice[n] = 2 I / (area_C +
 *      area_T), each rounded once to fp32; NaN where the denominator is 0.
 *   7. crossings[n] (int32) = the unordered pairs of curve edges (i, j), i + 1 < j, (i, j) not (0, P - 1) - pairs that share a
 *      vertex index are never tested - that cross properly: with det(p, q, s) = fma(q.x - p.x, s.y - p.y, -((q.y - p.y) (s.x -
 *      p.x))), edge i = (a0, a1) and edge j = (b0, b1), det(a0, a1, b0) and det(a0, a1, b1) have strictly opposite signs and so
 *      have det(b0, b1, a0) and det(b0, b1, a1).  An edge of no length never crosses.  crossings = 0 says that the curve is
 *      simple, and the row's I is then the reference's intersection.area; otherwise I is the winding-weighted value of item 5 (the
 *      reference rebuilds such a polygon by a rule of shapely's that is not restated here).  crossings reads no template.
 *   8. the association of the double sums is hint_hausdorff_run's.  Thread 64 v + l owns the curve edges i = 256 c + 64 v + l (c
 *      ascending) and, of every tile of 1024 template edges g = 1024 k + i, the edges i of the same form.  It adds to 0: for
 *      area_C its own curve edges' terms, c ascending; for area_T its own template edges' terms, tile after tile, c ascending;
 *      for I the pair terms in the order template edge g ascending and within it its own curve edges c ascending; for the
 *      crossings (an integer) the order does not matter.  The 64 lanes of a wavefront are added by a butterfly (lane distances
 *      32, 16, 8, 4, 2, 1); the four wavefronts are added in order.  The closing edge M_n - 1 -> 0 and every edge across a tile
 *      seam belong to the tile of their first vertex.  No float atomics, no counters.
 *   9. A row's outputs do not depend on n_rows, on where the row stands, on max_groups or on what the outputs held; two runs agree
 *      bit for bit.  A row with a value that is not finite among its curve points, its placed template vertices or its parameters,
 *      or whose ragged range is not 3..4096 points inside a_points, gets NaN in areas, iou and dice and -1 in crossings; it reads
 *      nothing outside its buffers, faults nothing and disturbs no other row.
 *   run              stream-ordered on the current device: one launch, no workspace, no host synchronisation, no allocation
 *                    (capturable).  Each output may be NULL, not all four.  When only crossings is asked the template is not
 *                    read: a_points and plus_params may then both be NULL.  max_groups: 0 = the default grid, otherwise the
 *                    workgroups at most.  Rejects, before any device call and naming the field: no output; both of a_points and
 *                    plus_params; neither when areas, iou or dice is asked; a_offsets or a_params without a_points; both or neither
 *                    of x and b_points; n_rows outside 1..2^30; with x, n_coeffs even or outside 1..25 (ignored with b_points);
 *                    n_points outside 3..1024; n_template < 3; a shared template of more than 4096 points, ragged ones of more
 *                    than 4096 n_rows in all; max_groups < 0; a pointer that is not 4-byte (a_offsets: 8-byte) aligned.
 *   workspace_bytes  0: no workspace is needed, so the descriptor names none.  For sizes run would reject (n_coeffs = 0 stands
 *                    for the given source; max_template_points is the largest M_n, 12 for plus_params) hint_last_error() says
 *                    why, otherwise it is left empty.
 *   geometry         host only, for the default grid: field 0 the workgroups, 1 the rows a workgroup has in flight (one), 2 the
 *                    template edges of an LDS tile, 3 the grid cap, 4 the tiles of max_template_points.  Workgroup w of G takes
 *                    rows w, w + G, ...  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_overlap_desc {
    const float* x;                        /* NULL, or [n_rows, 4 n_coeffs] row-major: the traced source */
    const float* b_points;                 /* NULL, or device float[n_rows, n_points, 2]: the given source */
    int64_t n_rows;
    int32_t n_coeffs, n_points;            /* K odd 1..25 (traced source), P 3..1024 */
    const float* a_points;                 /* NULL, or device float[n_template, 2] */
    const int64_t* a_offsets;              /* NULL (shared template), or device int64[n_rows + 1], 8-byte aligned */
    const float* a_params;                 /* NULL, or device float[n_rows, 4]: x, y, scale, angle */
    int64_t n_template;                    /* T: points in a_points */
    const float* plus_params;              /* NULL, or device float[n_rows, 9]: the template is the plus shape's outline */
    float* areas;                          /* NULL, or device float[n_rows, 3]: area_T, area_C, I */
    float* iou;                            /* NULL, or device float[n_rows] */
    float* dice;                           /* NULL, or device float[n_rows] */
    int32_t* crossings;                    /* NULL, or device int32[n_rows] */
    int32_t max_groups;
} hint_overlap_desc;
size_t hint_overlap_workspace_bytes(int64_t n_rows, int32_t n_coeffs, int32_t n_points, int64_t max_template_points);
int hint_overlap_run(const hint_overlap_desc* desc, void* stream);
int64_t hint_overlap_geometry(int64_t n_rows, int32_t n_points, int64_t max_template_points, int32_t field);

/* Correlation matrix and correlation MSE, the second number of the reference's test_likelihood (run_experiments.py:212-221:
 * the sample goes to the host, np.corrcoef(x.T) and np.nanmean(np.square(corr - corr_true)) run there; corr_true is the
 * np.corrcoef of a ground-truth sample, rejection_sampling.py:105-132).  For x fp32 [n, d], rows being samples, all in double:
 *   u = x - column mean,  S_ij = sum_rows u_i u_j,  r_ij = S_ij / (sqrt(S_ii) sqrt(S_jj)) clipped to [-1, 1]
 *   out = {mse, sum, count, nan_r}: sum of (r_ij - t_ij)^2 over the `count` entries where that difference is not NaN,
 *         mse = sum / count (NaN for count 0: np.nanmean's value), nan_r = NaN entries of r.  Without a target: {NaN, 0, 0, nan_r}.
 * NaN semantics are numpy's: a column of zero variance (n = 1: every column), or one holding a NaN or an inf, gives a NaN row and
 * column of r and changes no other entry.  corr is symmetric bit for bit.  Four launches on `stream`, no atomics: the same bits
 * on every run.  Every byte of out, of corr (when given) and of the first workspace_bytes the library asks for is written.
 *   hint_corr_workspace_bytes   bytes of workspace for a run (0 on bad sizes); never more than 68 MiB (d = 512, n > 16384), 2.3 MiB
 *                               at 10000 x 100.  Limits: 1 <= n <= 2^24, 1 <= d <= 512.
 *   hint_corr_job               the Gram launch's work items, host only: the rows are cut into slabs of R rows (R = 256 up to 64
 *                               slabs, more rows per slab beyond), and a job is one slab's 16 x 16 tile (ti, tj >= ti) of S.
 *                               j = -1: field 0 the job count, 1 the tile edge, 2 R, 3 the slab count; j >= 0: field 0 the job's
 *                               slab, 1 ti, 2 tj, 3 its first row, 4 its row count.  -1 on an error.
 * None of these has a caller's device buffer among its parameters: the buffers are named by the descriptor. */
typedef struct hint_corr_desc {
    const float* x;                        /* device float[n, d] row-major, 4-byte aligned */
    int32_t n, d;
    const double* target;                  /* NULL, or device double[d, d]: corr_true */
    double* corr;                          /* NULL, or device double[d, d]; target and corr are not both NULL */
    double* out;                           /* device double[4] */
    void* workspace; size_t workspace_bytes;      /* 16-byte aligned */
} hint_corr_desc;
size_t hint_corr_workspace_bytes(int32_t n, int32_t d);
int hint_corr_run(const hint_corr_desc* desc, void* stream);
int64_t hint_corr_job(int32_t n, int32_t d, int64_t j, int32_t field);

/* The lens-shape prior sampler: what feeds the evaluation pipeline (data.py:85-125 LensShapeModel.generate_lens_shape, sample_prior
 * and sample_joint - one polygon-library intersection and one DFT per row in a Python loop; rejection_sampling.py:76-85
 * prepare_samples runs it for 1e8 prior rows, data.py:466-489 prepare_data_loaders for the training and test sets).  A row has four
 * draws, u_r, u_t in [0, 1] and n_x, n_y standard normal:
 *   r0 = 1 + u_r, r1 = 2 r0, theta = 2 pi u_t, c1 = 0.8 (r0 + r1) (sin theta, cos theta)                          (data.py:87-93)
 *   A_j = r0 e_j, B_j = c1 + r1 e_j, e_j = (cos(2 pi j / 64), -sin(2 pi j / 64)), j = 0..63: the two clockwise 64-gons a
 *         default-resolution buffer() of a point stands for
 *   ring  = P, the A_j strictly inside B in A's clockwise order (one cyclic run), Q, the B_j strictly inside A in B's clockwise
 *         order, P again: the closed clockwise ring of A n B.  P and Q are the two edge-edge crossings, P the one where the
 *         boundary passes onto A.  THE ORDER OF THE RING'S VERTICES IS THIS LIBRARY'S DEFINITION: the reference takes whatever its
 *         polygon library returns, and that library is not available to pin it.  The closed ring has 31 or 32 points (the count
 *         depends on theta alone: 90.5 % / 9.5 %); the closing point stays in (data.py:98).
 *   ring -= mean(closed ring) + 0.5 (n_x, n_y)                                                                     (data.py:99)
 *   x     = the 20 floats flatten_coeffs(fourier_coeffs(ring, 5)) (data.py:30-33, :42-49), as hint_fcoef_desc states them
 * all in fp32: sin and cos of theta by sincospi(2 u_t); the figure is built at r0 = 1 and a centred point is
 * fma(r0, p - mean, -n / 2); the sums run in ring order.  tests/shapegen_oracle.py derives the distance to the exact value: at
 * most 153 u A per ring point and 187 u A per coefficient, u = 2^-24, A the row's largest centred coordinate magnitude; rows in
 * which a vertex lies within 2^-19 r0 of the other polygon's boundary may differ from the exact count by a vertex.
 * Draws: `draws` [n_rows, 4] = (u_r, u_t, n_x, n_y) as given, or (draws NULL) Philox4x32-10 with counter = {row lo, row hi, stream,
 * 0x4C454E53}, key = {seed lo, seed hi}, row = offset + i.  Stream 0: u_r = (float)c0 2^-32, u_t = (float)c1 2^-32, (n_x, n_y) = one
 * Box-Muller pair (r cos, r sin) of (min(((float)c2 + 1) 2^-32, 1), (float)c3 2^-32).  Stream 1: eps, the pair of (c0, c1): the
 * observation noise sample_joint adds.  A row depends on (seed, offset + i) only: a run cut into chunks at any boundaries gives
 * the bits of one call, and two runs agree bit for bit.  draws_out receives the draws used (either source).
 * A row whose u_r or u_t is outside [0, 1], or one of whose draws is not finite, is REJECTED: x = NaN, count 0, ring 0; it
 * disturbs no other row.  The workspace is int32[workspace_bytes / 4]: every word is written by a run and their sum is the
 * number of rejected rows (0 for every Philox run).
 *   run              stream-ordered on the current device: one launch, no host synchronisation, no allocation (capturable).
 *                    max_groups: 0 = the default grid, otherwise the workgroups at most.  Rejects, before any device call and
 *                    naming the field: a null desc, x or workspace; n_rows outside 1..2^30; offset + n_rows above 2^64 - 1;
 *                    max_groups < 0; draws, x, draws_out or workspace not 16-byte, ring or eps not 8-byte, counts not 4-byte
 *                    aligned; a workspace smaller than workspace_bytes says.
 *   workspace_bytes  0 (and an error message) for an n_rows run would reject.  Never decreases with n_rows; at most 32 KiB. */
typedef struct hint_lensgen_desc {
    int64_t n_rows;
    uint64_t seed, offset;
    const float* draws;                    /* NULL (Philox), or device float[n_rows, 4], 16-byte aligned */
    float* x;                              /* device float[n_rows, 20], 16-byte aligned */
    float* ring;                           /* NULL, or device float[n_rows, 32, 2]: the closed ring, centred, zero-padded */
    int32_t* counts;                       /* NULL, or device int32[n_rows]: points of the closed ring, 31 or 32 */
    float* eps;                            /* NULL, or device float[n_rows, 2] */
    float* draws_out;                      /* NULL, or device float[n_rows, 4], 16-byte aligned */
    void* workspace; size_t workspace_bytes;      /* 16-byte aligned */
    int32_t max_groups;
} hint_lensgen_desc;
size_t hint_lensgen_workspace_bytes(int64_t n_rows);
int hint_lensgen_run(const hint_lensgen_desc* desc, void* stream);

/* Points to Fourier coefficients (data.py:42-49 fourier_coeffs and :30-33 flatten_coeffs): the opposite direction of the traced
 * curves above.  For points [n_rows, p_max, 2], of which row i counts its first N = counts[i] (all p_max without counts), and
 * K = n_coeffs odd:
 *   a[c, m] = (1 / N) sum_n p[n, c] exp(-2 pi i m n / N), m = -K/2 .. K/2;  x[i] = [Re a[0, :], Re a[1, :], Im a[0, :], Im a[1, :]]
 * in fp32: for each |m| and axis, C = sum p cos(phi_n) and S = sum p sin(phi_n), phi_n = 2 pi ((|m| n) mod N) / N - the angle
 * reduced in integers, each twiddle the true value rounded once (sincospi in double) - fused multiply-adds onto the sum, n
 * ascending; Re a[+-m] = C / N, Im a[m] = -S / N, Im a[-m] = S / N.  Within (N + 2) u A of the exact value, A the row's largest
 * coordinate magnitude.  K <= N <= p_max is required of every row, so the reference's M = min(N // 2, M) never binds and the
 * output's width never depends on a row; a row with another count is REJECTED (x = NaN) and counted in the workspace as
 * hint_lensgen_desc's rows are.
 *   run              one launch, stream-ordered, capturable.  Rejects, before any device call and naming the field: a null desc,
 *                    points, x or workspace; n_rows outside 1..2^24; n_coeffs even or outside 1..25; p_max outside n_coeffs..1024;
 *                    max_groups < 0; points not 8-byte, counts or x not 4-byte, workspace not 16-byte aligned; a workspace
 *                    smaller than workspace_bytes says.
 *   workspace_bytes  0 (and an error message) for sizes run would reject.  Never decreases with n_rows; at most 128 KiB. */
typedef struct hint_fcoef_desc {
    const float* points;                   /* device float[n_rows, p_max, 2], 8-byte aligned */
    const int32_t* counts;                 /* NULL, or device int32[n_rows] */
    int64_t n_rows;
    int32_t p_max, n_coeffs;
    float* x;                              /* device float[n_rows, 4 n_coeffs] */
    void* workspace; size_t workspace_bytes;      /* 16-byte aligned */
    int32_t max_groups;
} hint_fcoef_desc;
size_t hint_fcoef_workspace_bytes(int64_t n_rows, int32_t p_max, int32_t n_coeffs);
int hint_fcoef_run(const hint_fcoef_desc* desc, void* stream);

/* The plus-shape sampler: prior, joint and targeted rows (data.py:176-252 PlusShapeModel.densify_polyline, generate_plus_shape,
 * sample_prior and sample_joint - one polygon-library union, one densify_polyline and one 25-coefficient DFT per row in a Python
 * loop; data.py:466-489 runs it for the training and test sets, rejection_sampling.py:76-85 for the 1e8-row prior,
 * rejection_sampling.py:113-127 in the rejection loop of the ground-truth conditional sample).  The plus model has no
 * forward_process: its labels y exist nowhere but here.  A row has nine draws, u_xl, u_yl, u_xw, u_yw, u_xs, u_ys, u_a in [0, 1]
 * and n_x, n_y standard normal.  Everything below is fp32 unless it says otherwise.
 *   1 parameters (data.py:190-202)  xlength = fma(2, u_xl, 3), ylength = fma(2, u_yl, 3); xwidth = fma(1.5, u_xw, 0.5), ywidth =
 *     fma(1.5, u_yw, 0.5); xshift = fma(3, u_xs, -1.5), yshift = fma(3, u_ys, -1.5); angle = (float)(pi / 2) u_a.  With a TARGET
 *     t = (cx, cy, angle, ratio), 0.25 <= ratio <= 4 (data.py:195-200, :216): xwidth = fma(2 - ratio / 2, u_xw, ratio / 2) when
 *     ratio >= 1, otherwise fma(2 ratio - 0.5, u_xw, 0.5); ywidth = xwidth / ratio; angle = t[2]; u_yw and u_a go unused (they are
 *     still drawn and still checked).  The bound on ratio keeps both widths in [0.5, 2], below the lengths.  t[0], t[1] are not read.
 *   2 local coordinates: the eight of plus_segments_from_params (best_shape_fit.py:28-29) without its 0.01 clamps, by the
 *     operations of hint_plus_desc item 1:  xleft = xshift - xlength / 2, xright = xshift + xlength / 2, xtop = xwidth / 2,
 *     xbottom = -xtop;  yright = ywidth / 2, yleft = -yright, ybottom = yshift - ylength / 2, ytop = yshift + ylength / 2.
 *   3 the union's ring.  THE ORDER OF THE RING'S VERTICES IS THIS LIBRARY'S DEFINITION: the reference takes whatever its polygon
 *     library returns, and that library is not available to pin it.  The ring is the corners of the union of the two boxes,
 *     clockwise, starting at the first corner met clockwise from the negative x axis; for the full plus this is the vertex order of
 *     plus_segments_from_params (:34-45).  Arm present: left xleft < yleft, right xright > yright, top ytop > xtop, bottom
 *     ybottom < xbottom; EQUALITY (measure zero) IS "ARM ABSENT".  Per quadrant, clockwise - upper-left shown, the other three
 *     follow by symmetry (upper-right, lower-right, lower-left, each in clockwise order):
 *         both arms       (xleft, xtop), (yleft, xtop), (yleft, ytop)
 *         left arm only   (xleft, xtop)
 *         top arm only    (yleft, ytop)
 *         neither         (yleft, ytop), (xleft, ytop), (xleft, xtop): the notch with its reflex corner
 *     12 corners (full plus, 73.0 % of the prior) or 8 (one arm missing, four patterns of 6.2 %; two adjacent arms missing, four of
 *     0.54 %); two opposite arms cannot be missing (lengths exceed widths).  No collinear vertices, no duplicates.
 *   4 densify_polyline(coords, 0.2) (data.py:176-186), as hint_plus_desc item 6 states it for 0.02: edge i runs from E = V_i to
 *     S = V_(i+1); len = max(|S.x - E.x|, |S.y - E.y|) (a difference of local coordinates: the ring is axis-aligned); count =
 *     max(1, rint((double)len / 0.2)), round half to even; point j is E when count = 1, otherwise fma(t, S, (1 - t) E) with
 *     t = (float)j / (float)(count - 1).  A vertex appears twice where both its edges have count >= 2, as in the reference.
 *     N = the sum of the counts: 54 <= N <= 106 from the perimeter's bounds; storage is 128 points a row.
 *   5 centring, rotation, offset (data.py:211-222): mean = (sum of the N dense points) / (float)N, the sum a fixed tree - sixteen
 *     partial sums s_k = p_k + p_(k+16) + .. (ascending), then s_0 + s_1 + .. + s_15 (ascending); p -= mean; p = p R, R = [[cos a,
 *     sin a], [-sin a, cos a]] with sincos in double of the fp32 angle, rounded once, by the operations of hint_plus_desc item 2
 *     (qx = fma(-py, sin, px cos), qy = fma(py, cos, px sin)); p += (0.5 n_x, 0.5 n_y).
 *   6 label (data.py:203, :211, :219, :222, :225): center = (-mean) R + 0.5 (n_x, n_y) by the same operations;
 *     y = (center_x, center_y, angle, xwidth / ywidth).
 *   7 x = the 100 floats flatten_coeffs(fourier_coeffs(points, 25)) (data.py:30-33, :42-49), as hint_fcoef_desc states them: the
 *     accumulators, n ascending, the angle reduced in integers, a[m] and a[-m] from one pair of sums, each twiddle the true
 *     value rounded once.
 * tests/plusgen_oracle.py derives the distance to the exact value, in units of u A (u = 2^-24, A the row's largest centred
 * coordinate magnitude, outline as it is written): a placed point 236, center 185, a coefficient 238 + N - worst-case chains; the
 * device's worst measured are 5.6, 1.9 and 6.6; a row with an arm shorter than 2^-20 or an edge whose
 * len / 0.2 lies within 2^-17 of a half-integer may differ from the exact ring by a point or a pattern.
 * Draws: `draws` [n_rows, 9] in the order above as given, or (draws NULL) Philox4x32-10 with counter = {row lo, row hi, stream,
 * 0x504C5553}, key = {seed lo, seed hi}, row = offset + i, or rows[i] where `rows` is given: stream 0 gives u_xl, u_yl, u_xw, u_yw
 * = (float)c 2^-32; stream 1 u_xs, u_ys, u_a (the fourth word is unused); stream 2 (n_x, n_y), the Box-Muller pair of (c0, c1) as
 * hint_lensgen_desc specifies it.  A row is a function of (seed, row, target) alone: chunks at any boundaries, the carry into the
 * counter's high word included, give the bits of one call; a gather by `rows` gives the bits the same rows have in a contiguous
 * call; two runs agree bit for bit.  draws_out receives the draws used (any source).
 * A row one of whose seven uniforms is outside [0, 1], or one of whose draws is not finite, is REJECTED: x = NaN, y = NaN, count
 * 0, corners 0, outline 0; it disturbs no other row.  The workspace is int32[workspace_bytes / 4]: every word is written by a run
 * and their sum is the number of rejected rows (0 for every Philox run), exactly as for hint_lensgen_run.
 *   run              stream-ordered on the current device: one launch, no host synchronisation, no allocation (capturable), no
 *                    atomics.  With x NULL (labels only) a row stops after the mean: no second pass, no transform.  THE STREAM IS A
 *                    FIELD OF THE DESCRIPTOR, unlike every other run of this header: the repository's frozen stream ledger
 *                    (tests/stream_cases.py) fails for any function declared here with a stream parameter that it has no row
 *                    for, and could not be given one when this entry point was added; tests/test_gpu_plusgen.py carries the
 *                    gated-stream test instead.  A consequence of that ledger, not a new convention.
 *                    max_groups: 0 = the default grid, otherwise the workgroups at most.  Rejects, before any device call and
 *                    naming the field: a null desc or workspace; x and y both NULL; n_rows outside 1..2^30; rows together with
 *                    draws; offset + n_rows above 2^64 - 1 (Philox without rows); max_groups < 0; a target entry that is not
 *                    finite or a ratio outside 0.25..4; x, y or workspace not 16-byte, rows or outline not 8-byte, draws, counts,
 *                    corners or draws_out not 4-byte aligned; a workspace smaller than workspace_bytes says.
 *   workspace_bytes  0 (and an error message) for an n_rows run would reject.  Never decreases with n_rows; at most 32 KiB. */
typedef struct hint_plusgen_desc {
    int64_t n_rows;
    uint64_t seed, offset;
    const uint64_t* rows;                  /* NULL, or device uint64[n_rows]: the Philox row of output row i (offset goes unused) */
    const float* draws;                    /* NULL (Philox), or device float[n_rows, 9]; not together with rows */
    const float* target;                   /* NULL, or HOST float[4] = (cx, cy, angle, ratio), read during the call */
    float* x;                              /* NULL, or device float[n_rows, 100], 16-byte aligned */
    float* y;                              /* NULL, or device float[n_rows, 4], 16-byte aligned; x and y are not both NULL */
    float* outline;                        /* NULL, or device float[n_rows, 128, 2]: the placed dense outline, zero-padded */
    int32_t* counts;                       /* NULL, or device int32[n_rows]: N, 54..106 */
    int32_t* corners;                      /* NULL, or device int32[n_rows]: corners + 16 arms - the low four bits are 8 or 12,
                                              arms = bit 0 left, 1 right, 2 top, 3 bottom (present) */
    float* draws_out;                      /* NULL, or device float[n_rows, 9] */
    void* workspace; size_t workspace_bytes;      /* 16-byte aligned */
    int32_t max_groups;
    void* stream;                          /* the hipStream_t the launch goes to (NULL: the null stream) */
} hint_plusgen_desc;
size_t hint_plusgen_workspace_bytes(int64_t n_rows);
int hint_plusgen_run(const hint_plusgen_desc* desc);

/* The trainable Householder permutation between blocks: what the reference's lens-shape and plus-shape configs put there as
 * HouseholderPerm(fixed=False, n_reflections=ndim) (configs/lens_shape/unconditional_hint_2_full.py:62-65 and thirteen siblings).
 * FrEIA is neither vendored by the reference nor available here, so THE PARAMETERISATION IS THIS LIBRARY'S DEFINITION (FrEIA parity
 * unpinned, as for the fixed orthogonal matrix).  For Vs fp32 [n, d], row i the vector v_i:
 *   H_i = I - 2 v_i v_i^T / (v_i . v_i),   W = H_0 H_1 .. H_(n-1), [d, d] row-major
 *   forward (transpose 0)  y = x W: a row meets H_0 first;   transpose 1  y = x W^T;   the log-determinant is 0
 * Limits: 1 <= d <= 128, 1 <= n <= 256, 1 <= B <= 2^22 (every element offset fits in 31 bits).  Nothing special happens for a zero
 * or non-finite v_i: the division gives NaN, and as every row of W passes through H_i all of W is NaN.  A non-finite row of x spoils
 * its own row of y only.
 *   op build  Vs -> W.  Row r of W is e_r taken through the reflections in order, w <- w - (2 (w . v_i) / (v_i . v_i)) v_i, IN DOUBLE:
 *             one wavefront per row, lane l keeping entries l and l + 64; a dot product is the lane's two terms added in that
 *             order, then a butterfly over the 64 lanes (distances 32, 16, .., 1); each entry is rounded to fp32 once.  One launch.
 *   op apply  x, W -> y, on v_mfma_f32_16x16x4_f32: tiles of 16 rows by 16 columns, W (or its transpose) staged once per workgroup in
 *             LDS with d padded to a multiple of 4 by zeros, the k-blocks of 4 added in ascending order.  A row's result depends
 *             on that row and W only: any split of the batch into calls gives the bits of one call.  Rows past B and columns
 *             past d are neither read nor written.  One launch.
 *   op grad   x, g_y, W, Vs -> any of g_x, g_W, g_V (a NULL output is not computed and not touched); at most three launches.
 *             g_x = g_y W^T (transpose 1: g_y W): apply with the other transpose flag.
 *             g_W = x^T g_y (transpose 1: g_y^T x), [d, d] fp32: the rows are cut into slabs of R rows (R = 256 up to 64 slabs,
 *             more rows per slab beyond, a multiple of 16); within a slab each of four wavefronts adds every fourth k-block of 4
 *             rows on the same MFMA, the four partial tiles are added in wavefront order and go to the workspace; the slabs of
 *             an entry are added in ascending order in double and rounded once.
 *             g_V [n, d] fp32 from that double sum G and Vs, in double, by one workgroup walking i = n-1 .. 0 with
 *             P = H_0 .. H_(i-1) and Gs = G (H_(i+1) .. H_(n-1))^T (reflections are involutions: P and Gs of step i - 1 are
 *             P H_(i-1) and Gs H_i, rank-one updates):  a = P v_i, b = Gs v_i, q = P^T b, qt = Gs^T a, s = v_i . v_i,
 *             g_(v_i) = -(2 / s) (q + qt) + (4 (a . b) / s^2) v_i.  O(d^2) per reflection; nothing is kept from the forward.
 *   run              stream-ordered on the current device, no host synchronisation, no allocation (capturable), no atomics: two
 *                    runs give equal bits.  Every byte of each output given is written and nothing outside them (and the
 *                    workspace).  THE STREAM IS A FIELD OF THE DESCRIPTOR, as in hint_plusgen_desc and for the same reason.
 *                    Rejects, before any device call and naming the field: a null desc; an unknown op; d outside its limits, n
 *                    (build, grad) or B (apply, grad) outside theirs; a required pointer NULL - Vs and W for build; x, W and y
 *                    for apply; g_y and W for grad, x as well when g_W or g_V is asked, Vs when g_V is, the workspace when
 *                    either is; grad with none of g_x, g_W, g_V; a device pointer not 4-byte or a workspace not 16-byte
 *                    aligned; a workspace smaller than workspace_bytes says; y aliasing x, g_x aliasing g_y.
 *   workspace_bytes  bytes a run of `op` needs: 0 for build and apply, which use none; for grad at most 4.3 MiB (d = 128,
 *                    B >= 16384).  For sizes run would reject: 0 and an error message.  Never decreases with B.
 *   geometry         host only: field 0 the slab's row count R of a grad run over B rows, 1 the number of slabs, 2 the tiles per
 *                    side of W.  -1 on an error. */
#define HINT_HOUSEHOLDER_BUILD 0
#define HINT_HOUSEHOLDER_APPLY 1
#define HINT_HOUSEHOLDER_GRAD 2
typedef struct hint_householder_desc {
    int32_t op;                            /* HINT_HOUSEHOLDER_BUILD / _APPLY / _GRAD */
    int32_t transpose;                     /* 0: y = x W; otherwise y = x W^T */
    int32_t B, d, n;
    const float* Vs;                       /* device float[n, d] */
    float* W;                              /* device float[d, d]: written by build, read by apply and grad */
    const float* x;                        /* device float[B, d] */
    float* y;                              /* device float[B, d] (apply) */
    const float* g_y;                      /* device float[B, d] (grad) */
    float* g_x;                            /* NULL, or device float[B, d] */
    float* g_W;                            /* NULL, or device float[d, d] */
    float* g_V;                            /* NULL, or device float[n, d] */
    void* workspace; size_t workspace_bytes;      /* 16-byte aligned */
    void* stream;                          /* the hipStream_t the launches go to (NULL: the null stream) */
} hint_householder_desc;
size_t hint_householder_workspace_bytes(int32_t op, int32_t B, int32_t d, int32_t n);
int hint_householder_run(const hint_householder_desc* desc);
int64_t hint_householder_geometry(int32_t B, int32_t d, int32_t field);

/* The m trainable permutations of one flow at once (FlowTrainer(learned_perms=True), hint_amd/train.py): every one of them has
 * the same d and n, its Vs, W, g_W, g_V and workspace slot lie a fixed stride of floats behind its predecessor's (the trainer's
 * arenas), and a training step needs all matrices before its forward pass and all g_V behind its backward pass.  The arithmetic is
 * hint_householder_run's, from the same device code: every output has the bits m single runs give.
 *   op build   W_j = H_0 .. H_(n-1) of Vs_j for j = 0 .. m-1: op build of hint_householder_run for each, in ONE launch.
 *   op rows    permutation j, the boundary in front of block j of the step's backward pass: g_x = g_y W_j^T (g_x may be NULL: not
 *              computed) and the slab partial tiles of x^T g_y into slot j of the workspace - the apply and Gram launches of a
 *              single grad run with transpose 0, the same slab geometry (hint_householder_geometry).  At most two launches.
 *   op finish  for every j: the slabs of slot j added in slab order in double -> g_W_j (g_W may be NULL), then g_(V_j) by the
 *              recurrence stated above in its order of operations, on W_j and Vs_j as they are now.  ONE launch, one workgroup per
 *              permutation: the m serial walks over the reflections run side by side.  Every slot must have had its op rows.
 *   run              stream-ordered on the current device, no host synchronisation, no allocation (capturable), no atomics: two
 *                    runs give equal bits.  Every byte of each output given is written (build: W_j [d, d]; rows: g_x; finish:
 *                    g_W_j [d, d], g_V_j [n, d] - the floats between two items of a stride are not touched) and nothing
 *                    outside them and the workspace.  THE STREAM IS A FIELD OF THE STRUCT, as in hint_householder_desc.
 *                    Limits: 1 <= m <= 64; d, n, B as for hint_householder_run; a stride is at most 2^30 floats.  Rejects, before
 *                    any device call and naming the field: a null job; an unknown op; m, d, n outside their limits, B (rows,
 *                    finish) outside its, j (rows) outside 0..m-1; a required pointer NULL - W for every op, Vs for build and
 *                    finish, x and g_y for rows, g_V for finish, the workspace for rows and finish; a device pointer not
 *                    4-byte or the workspace not 16-byte aligned; vs_stride < n d, w_stride < d d, gv_stride < n d, gw_stride
 *                    < d d (with g_W), ws_stride below a slot's floats or no multiple of 4; a workspace smaller than
 *                    (m - 1) ws_stride floats and one slot (workspace_bytes says it for dense slots); g_x aliasing g_y.
 *   workspace_bytes  m dense slots of hint_householder_workspace_bytes(grad, B, d, n) for rows and finish - the dense ws_stride
 *                    is a quarter of one slot's bytes - and 0 for build, which uses none.  For sizes run would reject: 0 and an
 *                    error message.  Never decreases with B or m. */
#define HINT_HOUSEHOLDER_MANY_BUILD 0
#define HINT_HOUSEHOLDER_MANY_ROWS 1
#define HINT_HOUSEHOLDER_MANY_FINISH 2
typedef struct hint_householder_many {
    int32_t op;                            /* HINT_HOUSEHOLDER_MANY_BUILD / _ROWS / _FINISH */
    int32_t m;                             /* permutations, 1..64 */
    int32_t j;                             /* rows: the permutation, 0..m-1 */
    int32_t B, d, n;
    const float* Vs; int64_t vs_stride;    /* device float[n, d] of permutation j at Vs + j * vs_stride */
    float* W; int64_t w_stride;            /* device float[d, d] at W + j * w_stride: written by build, read by rows and finish */
    const float* x;                        /* rows: device float[B, d], what permutation j was applied to */
    const float* g_y;                      /* rows: device float[B, d], the gradient of its product */
    float* g_x;                            /* rows: NULL, or device float[B, d] */
    float* g_W; int64_t gw_stride;         /* finish: NULL, or device float[d, d] at g_W + j * gw_stride */
    float* g_V; int64_t gv_stride;         /* finish: device float[n, d] at g_V + j * gv_stride */
    void* workspace; size_t workspace_bytes;      /* 16-byte aligned; slot j at (float*)workspace + j * ws_stride */
    int64_t ws_stride;
    void* stream;                          /* the hipStream_t the launches go to (NULL: the null stream) */
} hint_householder_many;
size_t hint_householder_many_workspace_bytes(int32_t op, int32_t m, int32_t B, int32_t d, int32_t n);
int hint_householder_many_run(const hint_householder_many* job);

/* Device-resident epochs: what stands between a resident table x [n_rows, d] (y [n_rows, dy]) and the training step - the
 * reference's DataLoader(TensorDataset(...), shuffle=True, drop_last=True) (data.py:484-487, :503-506: one __getitem__ per row and a
 * collate on the host) and the statistics of load_data_normalised (data.py:337-339).
 * THE ORDER OF AN EPOCH IS THIS LIBRARY'S DEFINITION: the reference's is torch's host generator and cannot be pinned.  It is a function
 * of (n_rows, seed, epoch, position) alone - no n_rows-sized randperm, no sort, no state:
 *   N = rows, 1 <= N <= 2^40.  epoch is a uint32.  seed is a uint64.
 *   h = max(1, ceil(bitlength(N-1) / 2)).  The domain is M = 4^h, so N <= M < 4N for N >= 2.  A value is split as v = L << h | R.
 *   The permutation is a balanced Feistel network of 4 rounds: (L, R) -> (R, L ^ F_r(R)).
 *   F_r(R) is the low h bits of word 0 of Philox4x32-10 with counter {R, r, epoch, 0x45504F43} and key {seed lo, seed hi}.
 *   Cycle walking: v = p; do v = feistel(v); while (v >= N).  source_row(p) = v.
 *   The walk is capped at 256 applications.  Every step succeeds with probability of at least 1/4, so a correct network exceeds
 *   the cap with probability below 1e-31.  A row that reaches the cap is flagged; the loop never runs on.
 *   shuffle = 0 is the identity.
 * Chunks of an epoch at any boundaries give the bits of one call; a data-parallel rank computes its own shard with no communication;
 * a run resumes mid-epoch from (seed, epoch, position).  hint_epoch_index is the host's twin, compiled from the same text
 * (hint_amd/csrc/hint_epochperm.hpp): the source row of position pos, or -1 and an error message for n_rows outside 1..2^40, pos
 * outside 0..n_rows-1 or a walk that reached the cap.
 *   op gather       out_x[i, :] = x[source_row(p_i), :] for i < count, and, with y, out_y[i, :] = y[source_row(p_i), :].  Position
 *                   p_i = first + i, or with block > 0 (a rank's share of every global batch) first + (i / block) * block_stride +
 *                   i % block.  x, y fp32 with row strides x_stride, y_stride (floats, 0..2^22; rows need no alignment beyond 4
 *                   bytes: no load is wider than a dword), 1 <= d <= 128, 0 <= dy <= 128 (dy > 0 exactly when y is given).  The
 *                   outputs are contiguous [count, d] and [count, dy].  Index arithmetic is 64-bit throughout.  indices_out
 *                   (may be NULL) receives the source rows; with it, x may be NULL (and y): the indices alone.  cursor (may be
 *                   NULL): device int64[2] = {epoch, first}, read only,
 *                   replacing the descriptor's epoch and first - a captured launch replays at a new position after a fill of the
 *                   cursor.  Every position must be < n_rows; with a cursor the host cannot check this, and a position >= n_rows
 *                   (or a cursor epoch outside 0..2^32-1, or first outside 0..n_rows-1) marks its row REJECTED, as a walk at its
 *                   cap does: the output row is NaN, indices_out -1, no other row is disturbed.  The workspace is
 *                   int32[workspace_bytes / 4]: every word is written by a run and their sum is the number of rejected rows, as
 *                   for hint_plusgen_run.  One launch.
 *   op moments      mean[j], std[j] (double[d] each) of column j over rows [first, first + count), in double: two passes over fixed
 *                   slabs of rows (at most 1024 slabs of at least 256 rows), a slab's column sum the sum of its threads' partial
 *                   sums (each over its rows ascending) in ascending order, the slabs added in ascending order; std =
 *                   sqrt(sum (x - mean)^2 / count), np.std with ddof 0.  Four launches.
 *   op standardize  out_x[i, j] = (float)(((double)x[i, j] - mean[j]) / std[j]) for rows [first, first + count) of the tables x
 *                   (x_stride) and out_x (out_stride >= d): IEEE double subtract and divide, rounded once.  out_x may be x.  A zero
 *                   std gives what numpy gives, NaN or +-inf; it is not guarded.  One launch.
 *   run              stream-ordered on the current device, no host synchronisation, no allocation (capturable), no atomics: two
 *                    runs give equal bits.  THE STREAM IS A FIELD OF THE DESCRIPTOR, as in hint_plusgen_desc and for the same reason.
 *                    max_groups: 0 = the default grid, otherwise the workgroups at most (gather, standardize).  Rejects, before
 *                    any device call and naming the field: a null desc or workspace; an unknown op; n_rows outside 1..2^40, count
 *                    outside 1..n_rows, d outside 1..128; max_groups < 0; x NULL (but for a gather of indices_out alone);
 *                    x_stride outside 0..2^22; first < 0; gather: dy
 *                    outside 0..128, out_x NULL, y without dy or dy without y, out_y NULL with y, y_stride outside its range,
 *                    block < 0 or 0 < block_stride < block; moments, standardize: mean or std NULL; standardize: out_x NULL,
 *                    out_stride outside d..2^22; first + count > n_rows (gather: the last position; with a cursor, its offset
 *                    from first); x, y, out_x or out_y not 4-byte, cursor, indices_out, mean or std not 8-byte, the workspace not
 *                    16-byte aligned; a workspace smaller than workspace_bytes says.
 *   workspace_bytes  bytes a run of `op` over `count` positions / rows needs (never 0 for sizes a run accepts: standardize uses
 *                    none and is given 16).  For sizes run would reject: 0 and an error message.  Never decreases with count; at
 *                    most 1 MiB (moments, d = 128), 32 KiB for gather. */
#define HINT_EPOCH_GATHER 0
#define HINT_EPOCH_MOMENTS 1
#define HINT_EPOCH_STANDARDIZE 2
typedef struct hint_epoch_desc {
    int32_t op;                            /* HINT_EPOCH_GATHER / _MOMENTS / _STANDARDIZE */
    int32_t shuffle;                       /* 0: source_row(p) = p */
    int32_t d, dy;
    uint32_t epoch;
    int32_t max_groups;
    int64_t n_rows;                        /* N: rows of the tables x and y */
    uint64_t seed;
    int64_t first, count;                  /* gather: the first position and the number of positions; otherwise the row range */
    int64_t block, block_stride;           /* gather: 0, 0 (contiguous positions), or 1 <= block <= block_stride */
    const float* x; int64_t x_stride;      /* device float table, row i at x + i * x_stride */
    const float* y; int64_t y_stride;      /* NULL (dy = 0), or the same for y */
    const int64_t* cursor;                 /* NULL, or device int64[2] = {epoch, first} */
    float* out_x; int64_t out_stride;      /* gather: device float[count, d] (out_stride unused); standardize: a table as x */
    float* out_y;                          /* gather with y: device float[count, dy] */
    int64_t* indices_out;                  /* NULL, or device int64[count] */
    double* mean;                          /* device double[d]: written by moments, read by standardize */
    double* std;                           /* likewise */
    void* workspace; size_t workspace_bytes;      /* 16-byte aligned */
    void* stream;                          /* the hipStream_t the launches go to (NULL: the null stream) */
} hint_epoch_desc;
int64_t hint_epoch_index(int64_t n_rows, uint64_t seed, uint32_t epoch, int32_t shuffle, int64_t pos);
size_t hint_epoch_workspace_bytes(int32_t op, int64_t n_rows, int64_t count, int32_t d);
int hint_epoch_run(const hint_epoch_desc* desc);

int hint_abi_version(void);
const char* hint_last_error(void);
/* what the library binary was built with and runs with: "libhint_amd abi N, gfx950, HIP x.y.z, clang ..., src <12 hex digits: hash
 * of the sources it was compiled from>[, knobs: HINT_X=v ...]" - the last part lists the HINT_* environment variables the library
 * found set (they change which kernels run).  Valid until the thread's next call; the HIP runtime of the machine that loads the
 * library may differ - bench.py prints both. */
const char* hint_build_info(void);

/* Diagnostics (process-wide; no effect on any result).  The general kernels touch the packed weights of what runs two
 * phases later into an LDS sink nobody reads (an L2 warm-up; on unless the environment says HINT_PF=0 when the library
 * first launches): hint_debug_set_prefetch(0 / 1) switches it for the launches that follow and returns the previous
 * setting - a launch already captured in a hipGraph keeps what it was captured with.  hint_debug_last_lds_bytes(backward)
 * = dynamic LDS bytes of the process's last forward / inverse (0) or backward part-A (1) launch; hint_debug_last_wl_shape(backward)
 * = the shape-table entry whose specialised instance that launch ran on, or -1 (a dynamic instance; HINT_WL_STATIC=0). */
int hint_debug_set_prefetch(int on);
/* The library reads its HINT_* environment variables once (the list: INTEGRATION.md); this re-reads them - for tests and A/B tools
 * that change the environment inside one process.  Plans already built keep what they were built with. */
int hint_debug_reload_knobs(void);
int32_t hint_debug_last_lds_bytes(int32_t backward);
int32_t hint_debug_last_wl_shape(int32_t backward);

#ifdef __cplusplus
}
#endif
#endif /* HINT_AMD_H */
