/*
 * bsx.h -- C-ABI of the MI355X (gfx950) Boolean-network state-update engine.
 *
 * This is the drop-in boundary for BoolSi's simulate / attract / target hot path.  The reference
 * (pure Python, /root/reference) has no FFI; the seam it offers is the per-batch function
 *     execute_task(task, solve, store, empty_results, n_to_find)        boolsi/mpi.py:498-544
 * with task = (batch seed, batch index, predecessor_node_lists, truth_tables)
 *                                                                       boolsi/batching.py:313-316
 * and the solver bound by configure_solve_simulation_problem            boolsi/mpi.py:351-376.
 * One bsx_run_* call does the work of execute_task over a contiguous range of the problem
 * index: enumerate -> adjust rules for fixed nodes -> solve -> store/aggregate.
 *
 * Conventions
 *   - plain C, caller-allocated host buffers, no callbacks, no torch / numpy types;
 *   - every function returns BSX_OK (0) or a negative bsx_status; bsx_last_error() gives text;
 *   - one handle per device; a handle is not thread-safe, distinct handles are independent;
 *   - there is NO CPU implementation behind this API: bsx_create fails without a gfx950 device.
 *
 * State layout: a state is W = ceil(n/64) uint64 words, node i = bit (i % 64) of
 * word i / 64, so that the reference's state code (model.py:131-149) is the little-endian
 * big integer formed by the words.
 */
#ifndef BSX_H
#define BSX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSX_MAX_NODES        256
#define BSX_MAX_WORDS        4      /* uint64 words per state / key */
#define BSX_MAX_PREDECESSORS 24
#define BSX_MAX_PERT_VARIATIONS 32
#define BSX_T_INF            UINT64_MAX   /* "no cap" for max_t / max_len (the CLI's inf) */
/* Networks of BSX_MAX_NODES < n <= BSX_MAX_NODES_WIDE nodes run on the wide-state family (DESIGN.md "Wide networks"):
 * simulate, trajectories, target and target summary through the entry points below, attract through
 * bsx_run_attract_wide only.  Their 'any' nodes must fit a bsx_index (at most 64 * BSX_MAX_WORDS) for every call that
 * enumerates; bsx_run_attract_sampled takes spaces with up to n 'any' nodes. */
#define BSX_MAX_NODES_WIDE   1024
#define BSX_MAX_STATE_WORDS  16     /* uint64 words per state / key of the wide family */
#define BSX_LUT_WIDE         3      /* bsx_network_info's lut_mode for a network lowered to the wide family */

typedef enum {
    BSX_OK = 0,
    BSX_ERR_INVALID = -1,        /* bad argument / inconsistent tables */
    BSX_ERR_NO_DEVICE = -2,      /* no gfx950 GPU, or HIP runtime failure at create */
    BSX_ERR_HIP = -3,            /* HIP call failed (text in bsx_last_error) */
    BSX_ERR_UNSUPPORTED = -4,    /* network / problem space exceeds an engine limit (BSX_MAX_*, variant >= 2^64) */
    BSX_ERR_TABLE_FULL = -5,     /* more distinct attractors / hits than the caller's capacity */
    BSX_ERR_STEP_LIMIT = -6,     /* a trajectory ran into the engine's internal step limit
                                    (only possible when max_t is BSX_T_INF or above that limit) */
    BSX_ERR_STATE = -7,          /* call order: network / problem space not set */
    BSX_ERR_COMM = -8,           /* RCCL: library not loadable, or an ncclXxx call failed */
    BSX_ERR_RANGE_TOO_LARGE = -9 /* the call is valid but its result does not fit THIS entry point's record (a 64-bit
                                    count / sum of a bsx_attr_rec overflowed): use bsx_run_attract2, or a smaller range */
} bsx_status;

/* Variation ranges = boolsi.constants.NodeStateRange (constants.py:23-30), digit -> state as in
 * batching.py:171-175. */
enum {
    BSX_RANGE_MAYBE_FALSE = 0,          /* '0?'   digit 0: absent, 1: 0           radix 2 */
    BSX_RANGE_MAYBE_TRUE = 1,           /* '1?'   digit 0: absent, 1: 1           radix 2 */
    BSX_RANGE_TRUE_OR_FALSE = 2,        /* 'any'  digit 0: 0,      1: 1           radix 2 */
    BSX_RANGE_MAYBE_TRUE_OR_FALSE = 3   /* 'any?' digit 0: absent, 1: 0, 2: 1     radix 3 */
};

typedef struct bsx_engine* bsx_handle;

/* Problem index I of the reference's mixed-radix enumeration (batching.py:10-46, 212-229), split
 * at the initial-state digits:  I = init_digits + variant * 2^n_any.
 *   init_digits: n_any binary digits, digit j = state of the j-th 'any' initial node (node order),
 *                packed little-endian into uint64 words (so I mod 2^n_any);
 *   variant:     the remaining digits (fixed-node variations, then perturbation variations) as one
 *                number, I >> n_any.  Must fit 64 bits. */
typedef struct {
    uint64_t init_digits[BSX_MAX_WORDS];
    uint64_t variant;
} bsx_index;

typedef struct { uint32_t node; uint32_t value; } bsx_fixed;              /* origin fixed node (model.py:31-49) */
typedef struct { uint32_t node; uint32_t range; } bsx_fixed_var;          /* fixed-node variation */
typedef struct { uint32_t t; uint32_t node; uint32_t value; } bsx_pert;   /* origin perturbation at time t >= 1 */
typedef struct { uint32_t t; uint32_t node; uint32_t range; } bsx_pert_var;

/* One aggregated attractor = reference AggregatedAttractor (attract.py:18-45) with the float
 * mean / M2 replaced by exact integer sums: mean = sum_l / count, M2 = sum_l2 - sum_l^2 / count. */
typedef struct {
    uint64_t key[BSX_MAX_WORDS];   /* min state code over the cycle (attract.py:296) */
    uint64_t length;               /* attractor length */
    uint64_t count;                /* frequency */
    uint64_t sum_l;                /* sum of trajectory_l = T_p + mu (attract.py:291-298) */
    uint64_t sum_l2_lo, sum_l2_hi; /* 128-bit sum of trajectory_l^2 */
} bsx_attr_rec;

/* Optional per-problem result of attract (what store_attractor receives, attract.py:374-402). */
typedef struct {
    uint64_t key[BSX_MAX_WORDS];
    uint64_t length;
    uint64_t trajectory_l;
    uint32_t found;                /* 0: no attractor within max_t / max_len */
    uint32_t pad;
} bsx_problem_rec;

/* target: one simulation that reached the target substate (target.py:109-133). */
typedef struct {
    uint64_t offset;               /* problem = first + offset */
    uint64_t t;                    /* first t >= T_p with state & mask == code */
} bsx_hit;

typedef struct {
    uint64_t problems;             /* problems processed */
    uint64_t state_steps;          /* steps the reference algorithm performs for them (S5-S7):
                                      t_stop per problem; simulate: max_t per problem */
    uint64_t executed_steps;       /* network updates the kernels actually executed */
    double   kernel_ms;            /* device time of the hot kernels (HIP events on the engine's stream) */
    double   total_ms;             /* wall time of the call incl. uploads, merge, downloads */
    uint32_t kernel_launches;
    uint32_t pad;
} bsx_stats;

int  bsx_create(bsx_handle* out, int device);
int  bsx_destroy(bsx_handle h);
const char* bsx_last_error(bsx_handle h);       /* h may be NULL: error of the last failed bsx_create */
const char* bsx_status_string(int status);
int  bsx_device_info(bsx_handle h, char* name, uint32_t name_cap, uint32_t* compute_units,
                     uint64_t* global_mem_bytes);

/* How the current network was lowered (valid after bsx_set_network): 32-bit words per state, gathered predecessor
 * slots of the mux tree, and where the gather table lives (0 HBM / L2, 1 LDS per state byte, 2 LDS per 4 state bits).
 * Together they name the kernel instantiations a run launches, e.g. k_attract_pool<words, slots, lut_mode, cube>. */
int  bsx_network_info(bsx_handle h, uint32_t* state_words32, uint32_t* mux_slots, uint32_t* lut_mode);

/* Network = (predecessor_node_lists, truth_tables) of the task tuple (batching.py:313-316).
 * pred_idx: predecessors of node i are pred_idx[pred_offsets[i] .. pred_offsets[i+1]) ascending
 * (input.py:796).  tt_words: table of node i starts at word tt_word_offsets[i] and has 2^k bits;
 * bit idx = output when predecessor j has state (idx >> j) & 1  (SURVEY.md S2). */
int  bsx_set_network(bsx_handle h, uint32_t n_nodes,
                     const uint32_t* pred_offsets, const uint32_t* pred_idx,
                     const uint32_t* tt_word_offsets, const uint64_t* tt_words);

/* Problem space = (origin_simulation_problem, simulation_problem_variations) of the batch seed
 * (batching.py:258-282, input.py:148-157); variation arrays in the reference's list order. */
int  bsx_set_problem_space(bsx_handle h, const uint64_t* origin_state_words,
                           const uint32_t* any_nodes, uint32_t n_any,
                           const bsx_fixed* fixed, uint32_t n_fixed,
                           const bsx_fixed_var* fixed_var, uint32_t n_fixed_var,
                           const bsx_pert* sched, uint32_t n_sched,
                           const bsx_pert_var* pert_var, uint32_t n_pert_var);

/* attract (attract.py:262-302 semantics for every problem of [first, first + count)):
 * aggregated table (unordered) into table[0..*n_out), problems without attractor counted in
 * *n_no_attractor.  per_problem (count entries) may be NULL.
 * A record's 64-bit count / sum_l and 128-bit sum_l2 must hold the result: BSX_ERR_RANGE_TOO_LARGE otherwise
 * (bsx_run_attract2 has wide records); count <= 2^32 with per_problem.  Large aligned ranges are not enumerated
 * problem by problem: the engine steps classes of problems that provably share their trajectory from some update
 * on (DESIGN.md "Cube collapse"). */
int  bsx_run_attract(bsx_handle h, const bsx_index* first, uint64_t count,
                     uint64_t max_t, uint64_t max_len,
                     bsx_attr_rec* table, uint32_t cap, uint32_t* n_out,
                     uint64_t* n_no_attractor, bsx_problem_rec* per_problem, bsx_stats* stats);

/* ---- attract over ranges of any size ("bsx_u128 first, count: N = 2^a * 3^b can exceed 2^64") ----------
 * The reference's N is a Python int (input.py:899-928) and ONE attract_master run covers it (attract.py:67-230);
 * bsx_run_attract2 is that call.  first / count are the flat problem index I of batching.py:212-229 and a number of
 * consecutive indices, 128 bits each; every sum of the record is wide enough for count = 2^128 problems of
 * trajectory_l < 2^64 each.  Words are little-endian (word 0 least significant). */
typedef struct { uint64_t lo, hi; } bsx_u128;

typedef struct {
    uint64_t key[BSX_MAX_WORDS];   /* min state code over the cycle (attract.py:296) */
    uint64_t length;               /* attractor length */
    bsx_u128 count;                /* frequency */
    uint64_t sum_l[3];             /* 192-bit sum of trajectory_l */
    uint64_t sum_l2[4];            /* 256-bit sum of trajectory_l^2 */
} bsx_attr_rec2;

typedef struct {
    bsx_u128 problems;             /* as bsx_stats, wide */
    bsx_u128 state_steps;
    uint64_t executed_steps;
    double   kernel_ms;            /* device time of all kernels of the call (HIP events on the engine's stream) */
    double   total_ms;
    double   dominant_ms;          /* ... of the dominant launches alone: the top level of every cube cascade */
    uint64_t dominant_executed_steps;  /* network updates those launches executed (the roofline's numerator) */
    uint32_t dominant_launches;
    uint32_t kernel_launches;
    uint32_t host_syncs;           /* times the host waited for the device inside the call (bsx_run_attract_wide on a
                                    * wide network: 1, or 2 for tables of more than 256 records, whatever the count;
                                    * kernel_ms there is taken from events around the whole chain of launches) */
    uint32_t lower_launches;       /* launches of the cascades' lower levels that had classes to work on ... */
    double   lower_ms;             /* ... their device time (first workgroup in to last one out, the device's 100 MHz clock) */
    uint64_t lower_executed_steps; /* ... and the network updates they executed */
} bsx_stats2;

/* Same semantics and table contents as bsx_run_attract (which stays, for ranges whose sums fit 64 bits).
 * A flat 128-bit index reaches every problem of spaces up to 2^128 problems; larger ones (more than 128 'any'
 * nodes) are reached through bsx_index with bsx_run_attract.  BSX_ERR_INVALID if first + count leaves the space. */
int  bsx_run_attract2(bsx_handle h, bsx_u128 first, bsx_u128 count,
                      uint64_t max_t, uint64_t max_len,
                      bsx_attr_rec2* table, uint32_t cap, uint32_t* n_out,
                      bsx_u128* n_no_attractor, bsx_stats2* stats);

/* attract through the functional graph (no reference analogue: the reference re-simulates every trajectory,
 * mpi.py:521-538): for spaces whose n <= 32 nodes are all 'any' (no variations, no perturbations) the network
 * is a function on 2^n states; successor array, pointer doubling and pointer jumping over 2^n-sized arrays in
 * HBM give every problem's (key, length, trajectory_l) without stepping trajectories.  Same results as
 * bsx_run_attract; other spaces return BSX_ERR_UNSUPPORTED. */
int  bsx_run_attract_fgraph(bsx_handle h, const bsx_index* first, uint64_t count,
                            uint64_t max_t, uint64_t max_len,
                            bsx_attr_rec* table, uint32_t cap, uint32_t* n_out,
                            uint64_t* n_no_attractor, bsx_stats* stats);

/* attract for networks of any supported size (n <= BSX_MAX_NODES_WIDE): bsx_run_attract2's semantics and sums, keys of
 * BSX_MAX_STATE_WORDS words.  For networks of the <= BSX_MAX_NODES family it returns what bsx_run_attract2 returns,
 * keys zero-extended; bsx_run_attract / bsx_run_attract2 / bsx_run_attract_fgraph return BSX_ERR_UNSUPPORTED for
 * wide networks.  count must fit 64 bits for wide networks.  There the records are aggregated on the device
 * (DESIGN.md "Wide networks"); the table comes back sorted by key words from key[0] up.  Device memory of the call
 * follows min(cap, count): about 600 bytes per possible attractor, kept on the handle; beyond 2^20 possible attractors
 * the records are aggregated on the host instead, as with BSX_WIDE_HOST_REDUCE=1. */
typedef struct {
    uint64_t key[BSX_MAX_STATE_WORDS];  /* min state code over the cycle */
    uint64_t length;
    bsx_u128 count;
    uint64_t sum_l[3];
    uint64_t sum_l2[4];
} bsx_attr_rec2w;

int  bsx_run_attract_wide(bsx_handle h, bsx_u128 first, bsx_u128 count,
                          uint64_t max_t, uint64_t max_len,
                          bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out,
                          bsx_u128* n_no_attractor, bsx_stats2* stats);

/* ---- attract, target and simulate over sampled initial conditions (no reference analogue: the reference enumerates) ----
 * For spaces too large to enumerate.  Sample j of seed `seed` is a problem of the current space; this definition is
 * NORMATIVE, part of the ABI, and implemented in boolsi_amd/csrc/bsx_sample.h.  All arithmetic is mod 2^64.
 *
 *     G      = 0x9E3779B97F4A7C15
 *     mix(z) : z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *     k0     = mix(seed + G)
 *     kb(b)  = mix(k0 + G * (b + 1))                     b = j >> 6   (a block of 64 samples)
 *     A(b,a) = mix(kb(b) + G * (a + 1))                  a = 0 .. n_any-1, the order of any_nodes
 *     U(j)   = mix(kb(j >> 6) + G * (n_any + 1 + (j & 63)))
 *
 *   - the a-th 'any' node of sample j has the state bit (j & 63) of A(j >> 6, a);
 *   - its variant number is (U(j) * V) >> 64, V the space's variant count: one 64 x 64 -> high multiply, whose bias is
 *     below V / 2^64 (a variant is drawn for floor or ceil of 2^64 / V values of U);
 *   - equivalently it is the flat index I(j) = sum of bit_a * 2^a + variant * 2^n_any of batching.py:212-229.
 * Hence a sampled call over [first, first + n) is a pure function of (seed, first, n), and disjoint sample ranges add up
 * to the call over their union (the multi-GPU partition rests on that).  Nothing here is an enumeration: the first n
 * samples of a seed are n independent draws, the first n indices of a space vary its low digits only.
 *
 * On the wide family a space may have up to n 'any' nodes.  With more than a bsx_index holds (64 * BSX_MAX_WORDS) only the
 * sampled calls below (and profile, correlations, transitions, which do not read the 'any' nodes) work on it; every entry
 * point that takes a bsx_index or a flat index returns BSX_ERR_UNSUPPORTED.  A space whose variant count does not fit
 * 64 bits is BSX_ERR_UNSUPPORTED here as everywhere. */

/* attract over samples [first_sample, first_sample + n_samples) of seed `seed` (definition above): bsx_run_attract_wide's
 * records, sums, order, capacity rules and statistics; count of a record = samples that reached it.  Works on handles of
 * both families with the same results (a handle of the <= BSX_MAX_NODES family lowers its network and space a second
 * time, on the first sampled call).  BSX_ERR_INVALID if first_sample + n_samples wraps. */
int  bsx_run_attract_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples,
                             uint64_t max_t, uint64_t max_len, bsx_attr_rec2w* table, uint32_t cap, uint32_t* n_out,
                             uint64_t* n_no_attractor, bsx_stats2* stats);
/* the problems behind listed sample numbers: states[q * W + w] = s(0) of sample samples[q], variants[q] (nullable) */
int  bsx_sample_problems(bsx_handle h, uint64_t seed, const uint64_t* samples, uint64_t n,
                         uint64_t* states, uint64_t* variants);

/* target and simulate over samples.  The three calls work on handles of both families with the
 * same results (the second lowering of bsx_run_attract_sampled), on spaces with up to n 'any' nodes, and are pure
 * functions of (seed, first_sample, n_samples) that add up over disjoint ranges.  BSX_ERR_INVALID if first_sample +
 * n_samples wraps, BSX_ERR_STATE without a network or a problem space, BSX_ERR_UNSUPPORTED for a space whose variant count
 * does not fit 64 bits.
 *
 * bsx_run_target_sampled: bsx_run_target_summary over samples [first_sample, first_sample + n_samples).  *n_hits is exact;
 * hist[b] = samples whose first hit is at t == b for b < hist_bins - 1, hist[hist_bins - 1] = at that time or later
 * (hist_bins may be 0, at most 2048); hits[0..*n_listed) = the first min(*n_hits, cap) hits in ascending sample order,
 * hits[].offset = sample - first_sample; cap may be 0, and then the host waits for the device once.  Times, state_steps
 * and the step limit are those of bsx_run_target_summary on a wide network: a trajectory that reaches the step limit
 * undecided (max_t BSX_T_INF, or at or beyond the limit of 2^24 lock steps / BSX_WIDE_STEP_LIMIT) makes the call return
 * BSX_ERR_STEP_LIMIT, and hist / hits are written only by a call that succeeds.  At most 2^40 samples per call. */
int  bsx_run_target_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples, uint64_t max_t,
                            const uint64_t* mask_words, const uint64_t* code_words,
                            uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap,
                            uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats);
/* bsx_run_simulate over samples [first_sample, first_sample + n_samples): the same three sinks (any may be NULL), layouts
 * and digest, p = sample - first_sample; a max_t at or above the step limit (2^30) is BSX_ERR_UNSUPPORTED. */
int  bsx_run_simulate_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples, uint64_t max_t,
                              uint64_t* trajectories, uint64_t* final_states, uint64_t* digests, bsx_stats* stats);
/* bsx_run_trajectories over listed samples: s(0..t_len[q]) of sample samples[q] (any 64-bit sample numbers, in any order)
 * at out[out_offsets[q] ..); used to materialise the simulations of sampled target hits.  Words of `out` that no
 * trajectory covers keep their value. */
int  bsx_run_trajectories_sampled(bsx_handle h, uint64_t seed, const uint64_t* samples, const uint64_t* t_len, uint64_t n,
                                  uint64_t* out, const uint64_t* out_offsets, bsx_stats* stats);

/* ---- damage spreading over sampled pairs of states: Derrida curves (no reference analogue) ----
 * How does a difference of n_flips nodes between two states grow or die over n_steps updates?  This definition is
 * NORMATIVE and implemented in boolsi_amd/csrc/bsx_sample.h; the notation is that of the sampled source above.  For
 * sample j of `seed`, kb = kb(j >> 6), lane = j & 63, h = n_flips, T = n_steps:
 *
 *   - x(0) is the sample's initial state as bsx_sample_problems gives it: 'any' nodes from A(b, a), the others from the
 *     origin;
 *   - free = the ascending list of the nodes that the origin does not fix, n_free of them;
 *   - for i = 0 .. h-1:   D(j, i) = mix(kb + G * (n_any + 65 + 64 i + lane))      (arguments past those of A and U)
 *                          p = (D(j, i) * (n_free - i)) >> 64
 *                          for every position c chosen earlier, in ascending order of c: if p >= c then p += 1
 *                          position p is chosen;
 *   - y(0) = x(0) with free[p] inverted for the h chosen positions (distinct by construction: d(0) = h exactly);
 *   - x(t+1) = F(x(t)), y(t+1) = F(y(t)) under the network's rules and the origin's fixed nodes only;
 *   - d_j(t) = popcount(x(t) ^ y(t)) for t = 0 .. T.
 *
 * Over samples [first_sample, first_sample + n_samples):  sum_d[t] = sum of d_j(t),  sum_d2[t] = sum of d_j(t)^2,
 * n_merged[t] = samples with d_j(t) == 0,  hist[t * (n_nodes + 1) + k] (nullable) = samples with d_j(t) == k.  A pure
 * function of (seed, first_sample, n_samples, n_flips, n_steps); disjoint sample ranges add up to their union.  Works on
 * handles of both families (the second lowering of bsx_run_attract_sampled).  The arrays are written only by a call that
 * succeeds; n_samples == 0 is BSX_OK with zeros written.  stats: problems = n_samples, state_steps = 2 * n_samples *
 * n_steps, executed_steps = the updates that ran (a group whose every pair has merged stops stepping: merged pairs stay
 * merged).
 *
 * Checked before anything is launched:  BSX_ERR_STATE without a network or a problem space;  BSX_ERR_INVALID if
 * first_sample + n_samples wraps, n_flips is 0, above n_free or above BSX_DAMAGE_MAX_FLIPS, or a required array is NULL;
 * BSX_ERR_RANGE_TOO_LARGE for more than 2^40 samples (the sums stay below 2^60);  BSX_ERR_UNSUPPORTED for a space with
 * fixed-node variations, perturbation variations or an origin perturbation schedule (the text says which: never a silent
 * reinterpretation), for n_steps > 65535, and for hist with more than 2^24 cells. */
#define BSX_DAMAGE_MAX_FLIPS 64
int  bsx_run_damage_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples,
                            uint32_t n_flips, uint32_t n_steps,
                            uint64_t* sum_d, uint64_t* sum_d2, uint64_t* n_merged, uint64_t* hist, bsx_stats* stats);

/* ---- node influence over samples: which node's flip reaches which node, and when (no reference analogue) ----
 * The influence matrix I(v -> i, t) = P(node i differs at step t | node v was inverted at step 0).  Its t = 1 slice is the
 * classical activity / influence of the rules, its row sums are the per-node sensitivities, its overall mean is the first
 * point of the Derrida curve; later slices show signalling range and the nodes whose perturbation never dies.  This
 * definition is NORMATIVE; the notation is that of the sampled source above, `free` is the ascending list of the nodes the
 * origin does not fix, as in damage.  A call lists n_sources distinct free nodes sources[s], in any order.  For source s
 * and sample j of `seed`, T = n_steps:
 *
 *   - x(0) is sample j's state, exactly as bsx_sample_problems gives it; y(0) is x(0) with node sources[s] inverted.  No
 *     random draw is involved;
 *   - x(t+1) = F(x(t)), y(t+1) = F(y(t)) under the network's rules and the origin's fixed nodes only;
 *   - D_j(t) = x(t) ^ y(t) for t = 1 .. T.
 *
 * Over samples [first_sample, first_sample + n_samples):
 *   influence[(s * T + (t - 1)) * n_nodes + i] = the number of samples with bit i of D_j(t) set;
 *   n_merged[s * T + (t - 1)] (nullable)       = the number of samples with D_j(t) == 0.
 * t = 0 is not stored: it is n_samples at i = sources[s] and 0 elsewhere.  A pure function of (seed, first_sample,
 * n_samples, sources, n_steps); disjoint sample ranges add up cell by cell; row s depends on sources[s] alone, so a call
 * over a subset or a permutation of the sources gives the same rows.  Works on handles of both families (the second
 * lowering of bsx_run_attract_sampled).  The arrays are written only by a call that succeeds; n_samples == 0 is BSX_OK with
 * zeros written.  stats: problems = n_sources * n_samples, state_steps = 2 * n_sources * n_samples * T, executed_steps =
 * the updates that ran (a group whose every pair has merged stops stepping: merged pairs stay merged); one host wait.
 *
 * Checked, in this order, before anything is launched:  BSX_ERR_STATE without a network or a problem space;
 * BSX_ERR_INVALID if influence or sources is NULL, n_sources or n_steps is 0, first_sample + n_samples wraps, or a source
 * is >= n, repeated or fixed by the origin (the text names the entry and the node);  BSX_ERR_RANGE_TOO_LARGE for n_samples
 * > 2^31 (a cell has 32 bits) or n_sources * n_samples > 2^40;  BSX_ERR_UNSUPPORTED for more than BSX_INFLUENCE_MAX_CELLS
 * cells (n_sources * T * n_nodes);  BSX_ERR_UNSUPPORTED for a space with fixed-node variations, perturbation variations or
 * an origin perturbation schedule (the text says which). */
#define BSX_INFLUENCE_MAX_CELLS (1ull << 26)
int  bsx_run_influence_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples,
                               const uint32_t* sources, uint32_t n_sources, uint32_t n_steps,
                               uint32_t* influence, uint64_t* n_merged /* nullable */, bsx_stats* stats);

/* ---- mutant screens over samples: knockouts and overexpressions in one call (no reference analogue) ----
 * Which attractors survive, which appear and how do the basin shares move when node v is held at 0 (knockout) or at 1
 * (overexpression), singly or in combinations?  This definition is NORMATIVE; the notation is that of the sampled source
 * above.
 *
 * A mutant is a list of 0 to BSX_SCREEN_MAX_NODES (node, value) pairs: the nodes distinct, below n and not fixed by the
 * origin, the values 0 or 1.  The empty list is the wild type.  Mutant m is mut_nodes[mut_offsets[m] .. mut_offsets[m + 1]).
 * Mutant m over sample j of `seed`:
 *
 *   - s(0) is sample j's state of the CURRENT space, exactly as bsx_sample_problems gives it: n_any, the ordinals a and
 *     the block keys are those of the current space whatever the mutant is, so every mutant runs on the wild type's
 *     initial states (common random numbers);
 *   - every listed node behaves as an origin fixed node does (model.py:31-49): it keeps its s(0) value at t = 0 and has
 *     `value` at every t >= 1;
 *   - everything else is bsx_run_attract_sampled with T_p = 0: found iff mu + lambda <= max_t, kept iff lambda <= max_len,
 *     key = the minimum state code over the cycle, l = mu.
 *
 * Hence the wild-type mutant gives bsx_run_attract_sampled's records, and a mutant whose nodes all have a constant initial
 * state gives the records of bsx_run_attract_sampled on the space that lists those nodes under `fixed nodes` (s(0) is NOT
 * forced: forcing it would break this identity).  The call is a pure function of (seed, first_sample, n_samples, mutant
 * list); disjoint sample ranges add up, per (mutant, key), to the call over their union.
 *
 * table[0 .. *n_out): records sorted by mutant, then by key words from word 0; counts and sums as in bsx_attr_rec2w.
 * n_no_attractor[m] (nullable) = n_samples - sum of the counts of mutant m.  stats: problems = n_mutants * n_samples, one
 * host wait (two when more than 256 records come back).  Works on handles of both families (the second lowering of
 * bsx_run_attract_sampled).  The caller's arrays are written only by a call that succeeds; n_samples == 0 is BSX_OK with
 * zeros written.  Reduced on the device only (BSX_WIDE_HOST_REDUCE is not read).
 *
 * Checked before anything is launched:  BSX_ERR_STATE without a network or a problem space;  BSX_ERR_INVALID if
 * first_sample + n_samples wraps, an array is NULL, the offsets do not ascend from 0, a mutant is longer than
 * BSX_SCREEN_MAX_NODES, a node is >= n, repeated within its mutant or fixed by the origin, a value is above 1, n_mutants is
 * 0 or above BSX_SCREEN_MAX_MUTANTS (the text names the mutant and the node);  BSX_ERR_UNSUPPORTED for a space with
 * fixed-node variations, perturbation variations or an origin perturbation schedule (the text says which);
 * BSX_ERR_RANGE_TOO_LARGE if n_mutants * n_samples exceeds 2^40;  BSX_ERR_TABLE_FULL for more distinct (mutant, key) pairs
 * than min(cap, 2^20). */
#define BSX_SCREEN_MAX_NODES   4
#define BSX_SCREEN_MAX_MUTANTS (1u << 20)
typedef struct { uint64_t mutant; bsx_attr_rec2w rec; } bsx_screen_rec;
int  bsx_run_screen_sampled(bsx_handle h, uint64_t seed, uint64_t first_sample, uint64_t n_samples,
                            const uint32_t* mut_offsets /* [n_mutants + 1] */, const bsx_fixed* mut_nodes,
                            uint32_t n_mutants, uint64_t max_t, uint64_t max_len,
                            bsx_screen_rec* table, uint64_t cap, uint64_t* n_out,
                            uint64_t* n_no_attractor /* [n_mutants], nullable */, bsx_stats2* stats);

/* target (target.py:109-133): hits in ascending offset order into hits[0..*n_hits); mask/code are W words
 * (target node set / target substate code, input.py:580-661). */
int  bsx_run_target(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                    const uint64_t* mask_words, const uint64_t* code_words,
                    bsx_hit* hits, uint64_t cap, uint64_t* n_hits, bsx_stats* stats);

/* target with an on-device summary instead of the full hit list, for sweeps whose hits cannot (and need
 * not) all travel to the host: *n_hits = number of problems that reach the target; hist[b] = those whose
 * first hit is at t == b for b < hist_bins - 1, hist[hist_bins - 1] = at that time or later (hist_bins may
 * be 0, at most 2048); hits[0..*n_listed) = the FIRST min(*n_hits, cap) hits in ascending offset order --
 * what the reference's -n option keeps (simulate.py:163-164, mpi.py:537-538); cap may be 0. */
int  bsx_run_target_summary(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                            const uint64_t* mask_words, const uint64_t* code_words,
                            uint64_t* hist, uint32_t hist_bins, bsx_hit* hits, uint64_t cap,
                            uint64_t* n_hits, uint64_t* n_listed, bsx_stats* stats);

/* simulate (simulate.py:97-131 == s(0..max_t) by plain stepping): any of the three sinks may
 * be NULL.  trajectories[(p * (max_t + 1) + t) * W + w], final_states[p * W + w], digests[p].
 * The digest is a checksum of the whole trajectory for runs too long to store (no reference counterpart):
 * FNV-1a (seed 0xCBF29CE484222325, prime 0x100000001B3) over the W words of X, then of Y, then of s(max_t),
 * where X = xor of s(0..max_t) and Y = xor of the s(t) with ((uint32_t)t * 0x9E3779B1) >> 31 == 1.  XORs of
 * whole states, so the bit-sliced kernels keep it per node row. */
int  bsx_run_simulate(bsx_handle h, const bsx_index* first, uint64_t count, uint64_t max_t,
                      uint64_t* trajectories, uint64_t* final_states, uint64_t* digests,
                      bsx_stats* stats);

/* trajectories s(0..t_len[q]) of listed problems (first + offsets[q]); used to materialise the
 * simulations of target hits.  out[q] starts at out_offsets[q] words. */
int  bsx_run_trajectories(bsx_handle h, const bsx_index* first, const uint64_t* offsets,
                          const uint64_t* t_len, uint64_t n, uint64_t* out,
                          const uint64_t* out_offsets, bsx_stats* stats);

/* Profile of listed attractors, the whole table in one call (what the per-attractor bsx_run_trajectories loop of a
 * host layer did): for each of n attractors given by (key state, length), walk the cycle from the key under the origin
 * problem's fixed nodes, without perturbations (attract.py:22-25: the listed states start at the key state).
 *   on_counts[q * n_nodes + i] = number of the cycle's `length` states in which node i is 1      (nullable)
 *   states[state_offsets[q] + t * W + w], t = 0 .. length-1, state 0 = the key                    (nullable; then state_offsets too)
 *   closed[q] = 1 iff f^length(key) == key                                                         (nullable)
 * keys: n rows of key_stride words, the first W of each row used (W = words per state of the current network,
 * 64-bit, little-endian as everywhere in this header).  Works for every supported network size.
 * Checked before anything is launched: network and problem space are set (BSX_ERR_STATE otherwise, as in every
 * bsx_run_* call); key_stride >= W; 1 <= length; no key bit at or above n_nodes; with `states`,
 * state_offsets non-null and the ranges [offset, offset + length * W) disjoint -- the end of the last one is the size of
 * `states` (BSX_ERR_INVALID otherwise); length below the family's step limit (2^30; on the wide family 2^24 lock steps,
 * or BSX_WIDE_STEP_LIMIT: BSX_ERR_STEP_LIMIT otherwise).  A key that is not on a cycle of the stated length is not an
 * error: closed[q] is 0 and the other outputs are the first `length` states from it.
 * The handle's problem space and cycle-state cache are left alone.  stats: problems = n, state_steps = sum of the
 * lengths.  The call makes one launch per BSX_PROFILE_CHUNK attractors (n <= 256 nodes) or per BSX_PROFILE_CHUNK_WIDE
 * attractors (wide family) and waits for the device once, whatever n is. */
#define BSX_PROFILE_CHUNK      (1ull << 22)
#define BSX_PROFILE_CHUNK_WIDE (1ull << 18)
int  bsx_run_attractor_profile(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths, uint64_t n,
                               uint32_t* on_counts, uint64_t* states, const uint64_t* state_offsets,
                               uint8_t* closed, bsx_stats* stats);

/* Node correlations of a whole attractor table: the matrix behind the frequency-weighted Spearman correlations of
 * attractor_analysis.find_node_correlations, in one call.  keys / key_stride / lengths / n, on_counts and closed are
 * those of bsx_run_attractor_profile; attractor q occurs frequencies[q] times.
 *   observation of node i in attractor q = on_count / length (IEEE double division of the two integers);
 *   per node column, rank2 = 2 W_less + W_equal + 1 (twice the average rank; W_less / W_equal = total frequency of the
 *   attractors with a smaller / an equal observation, q included) as an exact 64-bit integer; its weighted mean is
 *   T + 1 (T = sum of the frequencies), so d2 = rank2 - (T + 1) is an exact signed integer, converted to double once;
 *   s_matrix[a * n_nodes + b] = sum over q of frequencies[q] * d2[q][a] * d2[q][b]                     (required)
 *   ranks[q * n_nodes + i]    = rank2 / 2, the average weighted rank of attractor q in node i's column  (nullable)
 * rho_ab = S_ab / sqrt(S_aa S_bb) (the scale factors cancel); a node that is constant over the table has S_aa == +0
 * exactly.  s_matrix is symmetric bit for bit and the same bit for bit from run to run (upper-triangle tiles, no
 * floating-point atomics, partial sums of BSX_CORR_CHUNK attractors each added in chunk order).
 * Checked before anything is launched: everything bsx_run_attractor_profile checks; frequencies and s_matrix non-null,
 * every frequency at least 1 (BSX_ERR_INVALID); every frequency's high word 0 and T < 2^62 (BSX_ERR_RANGE_TOO_LARGE);
 * n * n_nodes <= BSX_CORR_MAX_CELLS (BSX_ERR_UNSUPPORTED).  n == 0 is BSX_OK with nothing written; n == 1 gives an
 * all-zero matrix.  Works for every supported network size; problem space, cycle-state cache and its mirror image are
 * left alone.  stats: those of the profile part, kernel_ms and kernel_launches with the correlation kernels added
 * (each column batch's sort counts as one launch).
 * Device memory, from the allocation sizes: 12 bytes per cell (on-counts, d2), 8 more with `ranks`, 32 bytes per cell
 * of one column batch (2^24 cells, or one column if that is more) plus the sort's own workspace of about 12 more,
 * 2 KiB per upper-triangle tile pair and chunk, 16 bytes per attractor.  At BSX_CORR_MAX_CELLS cells that is about
 * 43 GiB for 1024 nodes x 2^21 attractors with ranks (24 + 16 + 0.7 + 2 GiB of partials); the extreme of one node x
 * 2^31 attractors, whose only column is one batch, needs about 160 GiB. */
#define BSX_CORR_CHUNK     4096u
#define BSX_CORR_MAX_CELLS (1ull << 31)
int  bsx_run_node_correlations(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths,
                               const bsx_u128* frequencies, uint64_t n, double* s_matrix, double* ranks,
                               uint32_t* on_counts, uint8_t* closed, bsx_stats* stats);

/* Single-node flip transitions of a whole attractor table: is an attractor stable when one node is flipped once, and
 * if not, where does the network go and after how many steps?  keys / key_stride / lengths / n and closed are those of
 * bsx_run_attractor_profile.  F is the current network under the origin problem's fixed nodes, without perturbation
 * schedule or variations (what the profile walks); s[q][j] = F^j(key_q), j < length_q; the free nodes are those the
 * origin does not fix, n_free of them.
 * One flip per (q, j, i), i free: x_0 = s[q][j] XOR (1 << i), x_(t+1) = F(x_t); mu = the least t with x_t on a cycle C,
 * lambda' = |C|.  The flip is resolved iff mu + lambda' <= max_t (what bsx_run_attract reports as found for a problem
 * whose initial state is x_0 and whose last perturbation time is 0); BSX_T_INF resolves every flip.
 *   resolved, C is row d of the table:  edge (q, d), recovery time mu  (d == q: the flip returns)
 *   resolved, C is in no row:           edge (q, BSX_TRANS_OUTSIDE)
 *   not resolved:                       edge (q, BSX_TRANS_UNRESOLVED)
 * edges: one record per distinct (src, dst) with the number of flips and the sum of their mu (0 for the two
 *   pseudo-destinations), sorted by (src, dst); *n_edges = their number.  For every q the counts out of q add up to
 *   length_q * n_free.  More distinct edges than edge_cap: BSX_ERR_TABLE_FULL.
 * node_exits[q * n_nodes + i] = how many of the length_q flips of node i did not end as edge (q, q); fixed nodes 0.  (nullable)
 * closed[q] as in bsx_run_attractor_profile.                                                                          (nullable)
 * Refused before any flip is walked, with nothing written but the error text: everything bsx_run_attractor_profile
 * checks; edges and n_edges non-null, n <= 2^32 - 3 (BSX_ERR_INVALID); the sum of the lengths <= BSX_TRANS_MAX_STATES
 * (BSX_ERR_UNSUPPORTED); a row that is not closed, and two rows that share a state -- a duplicate row, or a length that
 * is a multiple of the true period -- (BSX_ERR_INVALID, the text names the row); a network on the wide-state family
 * (more than BSX_MAX_NODES nodes, or BSX_WIDE=1: BSX_ERR_UNSUPPORTED, the text says so).  n == 0 is BSX_OK with nothing
 * written.  A walk that reaches the internal step limit (2^30, or BSX_TRANS_STEP_LIMIT) undecided: BSX_ERR_STEP_LIMIT;
 * possible only when max_t is BSX_T_INF or beyond a third of that limit.
 * The handle's problem space, cycle journal and mirror image are left alone.  stats: problems = the number of flips,
 * state_steps = the sum of all sum_mu, executed_steps = the network updates the kernels ran (profile and walks),
 * kernel_launches / kernel_ms over all stages; the call waits for the device once.
 * Every output is exact and independent of the order in which the lanes arrive (integer atomics only).
 * Device memory, from the allocation sizes: per cycle state 8 W bytes of state (W = 64-bit words per state, at most 4), a
 * 4-byte row number and 8 to 16 bytes of table slots (4 bytes each, a power of two >= twice the states); 24 bytes per
 * edge-table slot (a power of two >= 2 * min(edge_cap, flips, n (n + 2)) + 2) and 24 per edge record; 9 + 8 W bytes per
 * row, 4 * n * n_nodes with node_exits.  At BSX_TRANS_MAX_STATES states of 256 nodes that is 8 + 1 + 2 = 11 GiB, and
 * 2^36 flips in launches of 2^28. */
#define BSX_TRANS_MAX_STATES (1ull << 28)
#define BSX_TRANS_OUTSIDE    0xFFFFFFFEu
#define BSX_TRANS_UNRESOLVED 0xFFFFFFFFu
typedef struct bsx_trans_edge {
    uint32_t src, dst;      /* rows of the table; dst may be BSX_TRANS_OUTSIDE / BSX_TRANS_UNRESOLVED */
    uint64_t count;         /* flips */
    uint64_t sum_mu;        /* sum of their recovery times */
} bsx_trans_edge;
int  bsx_run_attractor_transitions(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths, uint64_t n,
                                   uint64_t max_t, bsx_trans_edge* edges, uint64_t edge_cap, uint64_t* n_edges,
                                   uint32_t* node_exits, uint8_t* closed, bsx_stats* stats);

/* bsx_run_attractor_transitions for networks of every supported size: the same arguments, semantics, outputs, refusals
 * and statistics; keys are rows of key_stride >= W words with W up to BSX_MAX_STATE_WORDS.  On a network of the
 * <= BSX_MAX_NODES family the call forwards to bsx_run_attractor_transitions.  On the wide-state family (more than
 * BSX_MAX_NODES nodes, or BSX_WIDE=1) groups of flips walk in lock step, bit-sliced, and no state is looked up per
 * step: a flip's destination cycle is identified by its canonical key (the cycle's minimum state) in a table of the
 * rows' canonical keys, so a row may be listed from any state of its cycle.  Per flip that costs Brent's detector
 * (at most 3 (mu + lambda') + 2 steps), the mu pass (lambda' + 2 mu) and one lap of the cycle (lambda').
 * Refused as bsx_run_attractor_transitions refuses, before any flip is walked and with nothing written: a row that is
 * not closed; two rows on the same cycle, or a length that is a proper multiple of the true period (BSX_ERR_INVALID, the
 * text names the later row).  n == 0 is BSX_OK.  The step limit of this family counts lock steps of a group (2^24, or
 * BSX_WIDE_STEP_LIMIT); a max_t at or beyond a quarter of it is walked as unbounded (the result is still exact), and a
 * walk that reaches the limit undecided -- a flip's, or a row's own -- makes the call return BSX_ERR_STEP_LIMIT.
 * One host wait; the handle's problem space, cycle journal and mirror image are left alone.  stats as above, with
 * executed_steps = the trajectory updates of the profile, the rows' walks and the flips' walks.  One launch of the flips'
 * kernel per 2^22 flips (BSX_WTRANS_CHUNK changes that).
 * Device memory, from the allocation sizes: per cycle state 8 W bytes of state; per row 8 W bytes of canonical key,
 * 8 * key_stride of key, 8 bytes of period and mu, 8 to 16 bytes of row-key table (4 bytes a slot, a power of two >=
 * 2 n), 25 bytes of lengths, offsets, first-state index and closure, 4 * n_nodes with node_exits; 24 bytes per
 * edge-table slot (a power of two >= 2 * min(edge_cap, flips, n (n + 2)) + 2) and 24 per edge record; 4 * rows * L bytes
 * of spilled start states per workgroup (rows = n_nodes rounded up to 64, L <= 64 columns, a few workgroups per compute
 * unit).  At BSX_TRANS_MAX_STATES states of 1024 nodes the states alone are 32 GiB. */
int  bsx_run_attractor_transitions_wide(bsx_handle h, const uint64_t* keys, uint32_t key_stride, const uint64_t* lengths,
                                        uint64_t n, uint64_t max_t, bsx_trans_edge* edges, uint64_t edge_cap, uint64_t* n_edges,
                                        uint32_t* node_exits, uint8_t* closed, bsx_stats* stats);

/* Blocks until all work of the handle's stream is done (bench.py's timing fence). */
int  bsx_synchronize(bsx_handle h);

/* Multi-GPU merge step: one process per GPU, the problem index range-partitioned by the caller
 * ([r*N/G, (r+1)*N/G) for rank r), and ONE all-gather of the per-rank result tables at the end --
 * the counterpart of the reference master collecting its workers' batch results (mpi.py:290-330).
 * The collective is ncclAllGather (RCCL over xGMI) on the handle's stream.  The caller moves the
 * BSX_COMM_ID_BYTES unique id from rank 0 to the other ranks (any side channel: file, socket);
 * librccl.so is loaded on the first of these calls.
 *   bsx_comm_unique_id   rank 0 only: a fresh id (ncclGetUniqueId)
 *   bsx_comm_init        every rank, collectively: communicator of `world` ranks on the handle's device
 *   bsx_comm_allgather   every rank, collectively: recv[r * bytes_per_rank ..) = rank r's send buffer
 *                        (host buffers; staged through HBM by the library)
 *   bsx_comm_destroy     releases the communicator (bsx_destroy does it too) */
#define BSX_COMM_ID_BYTES 128
int  bsx_comm_unique_id(bsx_handle h, void* out, uint32_t cap);
int  bsx_comm_init(bsx_handle h, const void* unique_id, uint32_t id_bytes, int rank, int world);
int  bsx_comm_allgather(bsx_handle h, const void* send, uint64_t bytes_per_rank, void* recv);
int  bsx_comm_destroy(bsx_handle h);

#ifdef __cplusplus
}
#endif
#endif /* BSX_H */
