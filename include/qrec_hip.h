/*
 * qrec_hip.h -- C ABI of libqrec_hip.so, the MI355X (gfx950) implementation of QRec's
 * embedding-training hot path.
 *
 * The reference (Coder-Yu/QRec) is pure Python and has no FFI of its own; its only
 * extension seam is the Recommender template-method API (base/recommender.py:181-212).
 * Each entry point below replaces the body of one reference function; the Python model
 * classes in qrec_amd/ (and the stub a QRec maintainer would add)
 * bind these symbols with ctypes.  Plain C types only: pointers, sizes, scalars.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; qrec_last_error() gives the text
 *     (thread-local).  The reference reports errors with print+exit(-1)
 *     (util/config.py:8-10, base/iterativeRecommender.py:84-86); the Python wrapper maps
 *     error codes to that behaviour.
 *   - pointers named d_* are DEVICE pointers (from qrec_malloc or any HIP allocation,
 *     e.g. a torch tensor's data_ptr()); h_* are HOST pointers, borrowed for the call.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous on that stream unless stated otherwise.
 *   - embedding tables are row-major [rows][ld] with ld >= d, ld a multiple of 4 (fp32) and
 *     the pad columns zero; dtype is QREC_F32 or QREC_F64.
 *   - a handle is not thread-safe; one process drives one device.
 */
#ifndef QREC_HIP_H
#define QREC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QREC_OK 0
#define QREC_ERR_INVALID (-1)  /* bad argument */
#define QREC_ERR_HIP (-2)      /* a HIP runtime call failed */
#define QREC_ERR_NAN (-3)      /* loss is NaN/Inf (base/iterativeRecommender.py:84-86) */
#define QREC_ERR_UNSUPPORTED (-4)
#define QREC_ERR_NOT_SPD (-5)  /* a least-squares system is not positive definite (qrec_als_solve_rows) */

#define QREC_F32 0
#define QREC_F64 1
#define QREC_I32 2      /* collectives only */

/* ---- runtime ------------------------------------------------------------------------ */
int qrec_version(void);
const char *qrec_last_error(void);
int qrec_device_count(int *n);
/* Select the device for this process.  Deliberately NOT called from any constructor:
 * QRec builds model objects in the parent and forks per CV fold (QRec.py:76-89). */
int qrec_init(int device);
int qrec_device_info(char *name, int name_len, int *n_cu, int64_t *hbm_bytes, char *arch,
                     int arch_len);
int qrec_malloc(int64_t bytes, void **d_ptr);
int qrec_free(void *d_ptr);
int qrec_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes, void *stream);
int qrec_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes, void *stream);
int qrec_memcpy_d2d(void *d_dst, const void *d_src, int64_t bytes, void *stream);
/* Page-locked host memory and a device-to-host copy into it that only ENQUEUES (qrec_memcpy_d2h returns after the copy, i.e.
 * drains the stream): the host reads h_pinned after an event recorded behind the copy.  For the small read-backs a run-ahead
 * host needs while the stream carries on (the row counts of a sharded exchange plan, qrec_amd/dist.py). */
int qrec_host_alloc(int64_t bytes, void **h_ptr);
int qrec_host_free(void *h_ptr);
int qrec_memcpy_d2h_async(void *h_pinned, const void *d_src, int64_t bytes, void *stream);
int qrec_memset(void *d_dst, int byte, int64_t bytes, void *stream);
int qrec_stream_create(void **stream);
int qrec_stream_destroy(void *stream);
int qrec_stream_sync(void *stream);
int qrec_device_sync(void);
int qrec_event_create(void **ev);
int qrec_event_destroy(void *ev);
int qrec_event_record(void *ev, void *stream);
int qrec_event_sync(void *ev);
/* make `stream` wait (on the device) for work recorded in `ev` */
int qrec_stream_wait_event(void *stream, void *ev);
int qrec_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms);

/* ---- exact (bit-reproducible) sampler, host side ------------------------------------- *
 * Replays CPython's `random` (MT19937) word for word.  `state625` is
 * random.getstate()[1] (624 words + index) and is advanced in place so the Python host
 * can random.setstate() it back and stay in lock-step with the reference.            */

/* model/ranking/BPR.py:28-38: one negative per entry of the PositiveSet CSR, users in id
 * order, items in row order; redraw while the item is a positive of the user. */
int qrec_mt_bpr_sample_epoch(uint32_t *state625, const int64_t *h_pos_indptr,
                             const int32_t *h_pos_indices, int32_t n_users, int32_t n_items,
                             int32_t *h_j_out);
/* random.shuffle of a length-n list (base/iterativeRecommender.py:101,
 * base/deepRecommender.py:30).  h_perm (int64[n]) is permuted in place; NULL only
 * advances the generator. */
int qrec_mt_shuffle(uint32_t *state625, int64_t n, int64_t *h_perm);
/* DataSplit.dataSplit (util/dataSplit.py:9-25): one random() per row of the loaded file, in row order; is_test_out[k]
 * = 1 when random() < ratio.  Same draws as the reference's loop, so the -ap split is the reference's split. */
int qrec_mt_data_split(uint32_t *state625, int64_t n, double ratio, uint8_t *is_test_out);
/* base/deepRecommender.py:41-49 over rows already in shuffled order: one negative per
 * row, redraw while the item is in trainSet_u[user].  rated CSR rows must be sorted. */
int qrec_mt_pairwise_sample_epoch(uint32_t *state625, const int32_t *h_row_user, int64_t n_rows,
                                  const int64_t *h_rated_indptr, const int32_t *h_rated_sorted,
                                  int32_t n_items, int32_t *h_neg_out);

/* random.sample(range(n), k) (model/ranking/SGL.py:118-135: kept edges / dropped nodes of an
 * augmented sub-graph), same generator, same draws as CPython 3.10. */
int qrec_mt_sample_range(uint32_t *state625, int64_t n, int64_t k, int64_t *h_out);

/* ---- throughput sampler, device side -------------------------------------------------- *
 * Same distribution as BPR.py:35-37 (uniform over the items that are not positives of
 * the user, by rejection), counter-based Philox4x32-10 keyed by (seed, epoch, triplet
 * index): reproducible and order-independent, but NOT the CPython stream.
 * The stream is a contract: counter = {t_lo, t_hi, block, epoch_lo}, key = {seed_lo, seed_hi ^ epoch_hi}, block = 0, 1, ...;
 * the block's four words in order, candidate = word >> (32 - bit_length(n_items)), skipped when >= n_items or a positive of
 * d_row_user[t]; first survivor = d_j_out[t]; none in blocks 0 .. 4096: -1.  oracle/qrec_oracle.c orc_philox_bpr_sample
 * restates it (Philox pinned to Random123's known answers) and the kernel is held to it bit for bit.                        */
int qrec_philox_bpr_sample(const int64_t *d_pos_indptr, const int32_t *d_pos_sorted,
                           const int32_t *d_row_user, int64_t n, int32_t n_items, uint64_t seed,
                           uint64_t epoch, int32_t *d_j_out, void *stream);

/* Throughput mode of the pairwise (TF-path) models, base/deepRecommender.py:29-52 on the device: the epoch's row order
 * from qrec_random_permutations (a uniform shuffle, one device sort), the rows gathered into that order here, one
 * negative per row from qrec_philox_bpr_sample with the rated CSR as the exclusion set.  Same distribution as
 * shuffle + choice-with-rejection, not the CPython stream.                                                          */
int qrec_gather_pairs(const int32_t *d_perm, const int32_t *d_u, const int32_t *d_i, int64_t n, int32_t *d_u_out,
                      int32_t *d_i_out, void *stream);

/* ---- BPR SGD: model/ranking/BPR.py:45-53 --------------------------------------------- */

/* Order-exact mode: the n triplets are applied strictly one after another, in array
 * order, each seeing all earlier writes -- the reference's semantics.  One wavefront
 * walks the list (the dependency chain of an epoch is ~n/6 long).
 * *d_loss (double) receives sum(-log(sigmoid(x))) (overwritten).                        */
int qrec_bpr_sgd_ordered(void *d_P, void *d_Q, int dtype, int32_t d, int32_t ld,
                         const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int64_t n,
                         double lr, double regU, double regI, double *d_loss, void *stream);

/* Order-exact mode beyond one wavefront.  The negatives are drawn before the first update (sampling never looks at the
 * embeddings), so the epoch's dependence DAG -- triplet t waits for the previous toucher of P[u], Q[i], Q[j], nothing
 * else -- is known up front.  qrec_bpr_exact_schedule (host) list-schedules the triplets, in the reference's order, into
 * steps of at most `width` mutually independent triplets and records for every row where its current value will be
 * (LDS forwarding slot of one of the last two steps, or the table); qrec_bpr_sgd_scheduled executes the steps with one
 * workgroup of `width` wavefronts, one barrier per step.  Every row sees exactly the reference's sequence of updates:
 * results equal qrec_bpr_sgd_ordered's bit for bit (same per-triplet arithmetic), the loss up to its summation order.
 *   h_entries   : int32[n][8] out, step-major: {u, i, j, t, src_P, src_Qi, src_Qj, 0}
 *   h_step_off  : int32[n + 1] capacity out; entries of step s are [h_step_off[s], h_step_off[s+1])
 *   width       : <= qrec_bpr_exact_width(dtype, d) (what the CU's LDS holds), <= QREC_EXACT_MAX_WIDTH
 *   d_xlog      : table-dtype[n + QREC_EXACT_XLOG_PAD] scratch (x per triplet, then the dummy rows idle wavefronts work on),
 *   d_scratch   : double[QREC_EXACT_SCRATCH_WORDS], zero before first use */
#define QREC_EXACT_MAX_WIDTH 16       /* a power of two: a source code is ((dist - 1) * 16 + slot) * 4 + row, or -1 = the table */
#define QREC_EXACT_XLOG_PAD (16 * 256 + 64)
#define QREC_EXACT_SCRATCH_WORDS 130
int qrec_bpr_exact_width(int dtype, int32_t d, int32_t *width);
int qrec_bpr_exact_schedule(const int32_t *h_u, const int32_t *h_i, const int32_t *h_j, int64_t n, int32_t n_users,
                            int32_t n_items, int32_t width, int32_t *h_entries, int32_t *h_step_off, int64_t *n_steps);
int qrec_bpr_sgd_scheduled(void *d_P, void *d_Q, int dtype, int32_t d, int32_t ld, const int32_t *d_entries,
                           const int32_t *d_step_off, int64_t n_steps, int32_t width, int64_t n, double lr, double regU,
                           double regI, void *d_xlog, double *d_scratch, double *d_loss, void *stream);
/* Four triplets per wavefront (round 3; rows of 16, 32, 64 or 128 elements): a triplet on the 16 lanes of one DPP row, rows handed
 * on in registers or through the table, nothing in LDS (bpr_exact.hip).  Same order, same values as qrec_bpr_sgd_scheduled up to
 * the last bits (own summation tree and exp: 1e-13 apart in fp64); identical bits across widths.  2.4 x the steps per second.
 *   qrec_bpr_exact_kind       : which kernel serves (dtype, ld, width): 0 = qrec_bpr_exact_schedule + qrec_bpr_sgd_scheduled
 *                               (above), 1 = the three calls below; slots = 4 * ceil(width / 4) for kind 1.
 *                               Env QREC_EXACT_KERNEL=w64 forces 0 (measurement).
 *   qrec_bpr_exact_schedule_reg : host; arguments and entry format of qrec_bpr_exact_schedule, but h_step_off needs 3 n + 2
 *                               entries (steps may stay empty: n_steps <= 3 n).  A user's run stays on one slot and hands P[u]
 *                               on in that group's registers (src_P = -2); every other row is read from the table, so
 *                               touches of a row by different slots are kept >= 3 steps apart.  Entry word 7 = bit 0 (P goes
 *                               on in registers: no table store) | slot << 8 | 0x1000.
 *   qrec_bpr_exact_expand     : d_entries / d_step_off (device copies of that schedule) -> the fixed-width layout the kernel
 *                               reads: d_wide int32[(n_steps + QREC_EXACT_WIDE_PAD) * slots * 8], QREC_EXACT_WIDE_LEAD empty
 *                               steps in front, empty slots u = -1;
 *   qrec_bpr_sgd_scheduled_wide : the epoch; d_xlog / d_scratch / d_loss as above.  The tables are addressed through
 *                               bounds-checked 32-bit offsets: each of P, Q below 4 GiB (else kind 0).                        */
#define QREC_EXACT_WIDE_PAD 16
#define QREC_EXACT_WIDE_LEAD 4
int qrec_bpr_exact_kind(int dtype, int32_t ld, int32_t width, int32_t *kind, int32_t *slots);
int qrec_bpr_exact_schedule_reg(const int32_t *h_u, const int32_t *h_i, const int32_t *h_j, int64_t n, int32_t n_users,
                                int32_t n_items, int32_t width, int32_t *h_entries, int32_t *h_step_off, int64_t *n_steps);
int qrec_bpr_exact_expand(const int32_t *d_entries, const int32_t *d_step_off, int64_t n_steps, int32_t slots, int32_t *d_wide,
                          void *stream);
int qrec_bpr_sgd_scheduled_wide(void *d_P, void *d_Q, int64_t n_users, int64_t n_items, int dtype, int32_t d, int32_t ld,
                                const int32_t *d_wide, int64_t n_steps, int32_t slots, int64_t n, double lr, double regU, double regI,
                                void *d_xlog, double *d_scratch, double *d_loss, void *stream);

/* Throughput mode (fp32): triplets are cut into chunks of `chunk` consecutive entries;
 * one 16-lane (d<=64) / 32-lane (d<=128) group owns a chunk, keeps P[u] in registers
 * along a user run, and applies every row update as an atomic add of the exact
 * per-sample delta, so no update is lost; concurrent chunks read rows that may lag by
 * the in-flight updates (Hogwild).  grid_groups = number of groups in flight (0 = library
 * default: one 256-thread block per CU); with grid_groups==1 the kernel degenerates to the
 * sequential recurrence.  *d_loss (double) is ACCUMULATED into (zero it first).  n_users / n_items = rows of
 * d_P / d_Q: tables below 4 GiB are addressed through a buffer descriptor of exactly that size (a row id past the
 * end is dropped by the hardware bounds check), larger ones through 64-bit addresses (2-5% slower).
 * `variant` selects the memory policy (QREC_HW_*), 0 = library default.                  */
#define QREC_HW_DEFAULT 0
#define QREC_HW_PLAIN_RMW 1     /* plain loads, plain stores (racy read-modify-write)     */
#define QREC_HW_SC1_RMW 2       /* sc1 loads, sc1 write-through stores                    */
#define QREC_HW_ATOMIC 3        /* plain loads, f32 atomic-add deltas                     */
#define QREC_HW_SC1_ATOMIC 4    /* sc1 loads, f32 atomic-add deltas                       */
#define QREC_HW_P_RMW 5         /* item-major only: P[u] by sc1 load + sc1 store (racy), Q[i] / Q[j] by atomic deltas */
#define QREC_HW_PQ_RMW 6        /* item-major only: P[u] and Q[j] by sc1 load + sc1 store (measurements)              */
#define QREC_HW_FIXED 7         /* item-major only: atomic deltas as 32-bit INTEGER adds on fixed-point tables (see below)          */
int qrec_bpr_sgd_hogwild(float *d_P, float *d_Q, int64_t n_users, int64_t n_items, int32_t d, int32_t ld, const int32_t *d_u,
                         const int32_t *d_i, const int32_t *d_j, int64_t n, int32_t chunk,
                         int32_t grid_groups, float lr, float regU, float regI, double *d_loss,
                         int variant, const double *d_driver_state, void *stream);

/* The same Hogwild epoch, ITEM-major: the caller passes the triplets sorted by positive item (stable
 * within an item); Q[i] stays in registers along an item run (flushed as one atomic delta and re-read
 * every `flush_every` triplets), P[u] and Q[j] take the per-sample atomic deltas.  Moves the
 * per-triplet atomics off the hot item rows (Zipf 0.6) onto user rows (Zipf 0.4) and uniform
 * negatives, which the L2 atomic units retire ~25% faster.  Chunks are visited in a golden-ratio
 * stride order so that the chunks of one hot item are spread over the epoch.  With grid_groups == 1
 * and chunk order aside, each row still sees exactly the reference recurrence.
 * `variant`: QREC_HW_DEFAULT / QREC_HW_ATOMIC = the above.  QREC_HW_P_RMW (round 6): P[u] is read with sc1 loads and written back
 * with sc1 write-through stores instead of atomic deltas -- one atomic row update per triplet instead of two (0.63-0.64 of the
 * HBM roofline instead of 0.43-0.46), at the price that a P[u] update landing between another group's load and store of the same
 * row is lost.  The expected share of such updates is the collision density c = groups in flight x sum_u (n_u / n)^2; the host
 * takes this variant only where c <= 0.01 (qrec_amd/engine.py resolve_p_update; measured Recall@20 gaps by c in DESIGN.md s5.1).
 * QREC_HW_FIXED: the atomic-delta policy with the deltas added as integers, which the L2 atomic units retire faster than float adds.
 * The call expects both tables as int32 = rint(x * 2^26) (range +-32, quantum 1.5e-8) and needs d_driver_state: an epoch is
 * qrec_bpr_fixed_convert_in, this call, qrec_epoch_close_fixed; outside those three the tables are fp32.  Nothing wraps silently: a
 * value with |x| >= 16 or a NaN, at convert-in or produced by a step, sets d_driver_state[QREC_DRV_FAILED] (the one thing this
 * variant writes there); the close still writes the tables back as fp32 and the enqueued epochs behind it are no-ops.  An element
 * out of range at convert-in saturates; one that a step of a failed epoch carried past +-32 (its delta is added in two's complement)
 * may have wrapped. */
int qrec_bpr_sgd_hogwild_item_major(float *d_P, float *d_Q, int64_t n_users, int64_t n_items, int32_t d, int32_t ld,
                                    const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int64_t n, int32_t chunk,
                                    int32_t grid_groups, int32_t flush_every, float lr, float regU, float regI,
                                    double *d_loss, int variant, const double *d_driver_state, void *stream);
/* Device-resident epoch close of the numpy-path models: model/ranking/BPR.py:40 (loss += regU*sum(P*P) +
 * regI*sum(Q*Q)) followed by isConverged / updateLearningRate (base/iterativeRecommender.py:56-63,88-104),
 * so that a run can be enqueued epoch after epoch without a host round trip.
 *   d_stats : double[QREC_STATS_WORDS], zero before the first epoch: [0] the epoch's sum(-log sigma) (the SGD
 *             kernels accumulate into it; cleared again by the call), [1] sum P*P, [2] sum Q*Q (left for the
 *             caller), [3] ticket counter, then the per-block partial sums.
 *   d_state : double[QREC_DRV_WORDS], the bold-driver state below; initialise LR, everything else 0.
 *   d_log   : optional double[log_capacity][QREC_DRV_LOG_WORDS] = {loss, lr used, sum(-log sigma),
 *             lastLoss - loss, sum P*P, sum Q*Q, -, -} per epoch.
 * A SGD entry point given d_driver_state takes its learning rate from d_state[QREC_DRV_LR] and becomes a
 * no-op once CONVERGED or FAILED is set (tol = 1e-3 in the reference; 0 never converges; max_lr <= 0 = no cap). */
#define QREC_DRV_LR 0         /* learning rate of the NEXT epoch (lRate)             */
#define QREC_DRV_LAST_LOSS 1  /* lastLoss                                            */
#define QREC_DRV_EPOCHS 2     /* epochs closed so far                                */
#define QREC_DRV_CONVERGED 3  /* 1 once |lastLoss - loss| < tol                      */
#define QREC_DRV_FAILED 4     /* non-zero once the loss is NaN/Inf (the reference exits), or a QREC_HW_FIXED epoch left its range */
#define QREC_DRV_WORDS 8
#define QREC_DRV_LOG_WORDS 8
#define QREC_STATS_MAX_BLOCKS 256
#define QREC_STATS_PARTIALS 8
#define QREC_STATS_WORDS (QREC_STATS_PARTIALS + 2 * QREC_STATS_MAX_BLOCKS)
int qrec_epoch_close(const void *d_P, int64_t p_rows, const void *d_Q, int64_t q_rows, int dtype, int32_t ld,
                     double *d_stats, double *d_state, double regU, double regI, double max_lr, double tol,
                     double *d_log, int64_t log_capacity, void *stream);
/* The epoch boundary of a QREC_HW_FIXED epoch (fp32 tables only).  qrec_bpr_fixed_convert_in: both tables fp32 -> int32 in place,
 * a no-op once CONVERGED or FAILED.  qrec_epoch_close_fixed: qrec_epoch_close, reading the integers and writing fp32 back in place in
 * the same pass (no launch more than the float close); sum P*P and sum Q*Q are those of the fp32 values it leaves. */
int qrec_bpr_fixed_convert_in(float *d_P, int64_t p_rows, float *d_Q, int64_t q_rows, int32_t ld, double *d_state, void *stream);
int qrec_epoch_close_fixed(float *d_P, int64_t p_rows, float *d_Q, int64_t q_rows, int32_t ld, double *d_stats, double *d_state,
                           double regU, double regI, double max_lr, double tol, double *d_log, int64_t log_capacity, void *stream);
/* The two halves, for runs whose loss terms are summed over ranks in between (one process per GPU): qrec_epoch_sums
 * leaves sum P*P / sum Q*Q in d_stats[1..2] (d_state may be NULL; a converged/failed state makes it a no-op), the
 * caller all-reduces d_stats[0..1] (sum(-log sigma) and sum P*P add up over user shards, Q is replicated), and
 * qrec_epoch_decide takes the reference's decision from d_stats[0..2] exactly as qrec_epoch_close does. */
int qrec_epoch_sums(const void *d_P, int64_t p_rows, const void *d_Q, int64_t q_rows, int dtype, int32_t ld,
                    double *d_stats, const double *d_state, void *stream);
int qrec_epoch_decide(double *d_stats, double *d_state, double regU, double regI, double max_lr, double tol,
                      double *d_log, int64_t log_capacity, void *stream);
/* one table's (deterministic) sum of squares into d_stats[slot], slot 1 = sum P*P, 2 = sum Q*Q; the other slot is left alone */
int qrec_epoch_sum_table(const void *d_X, int64_t rows, int dtype, int32_t ld, double *d_stats, int slot,
                         const double *d_state, void *stream);

/* Rating-prediction MF family, order-exact: variant 0 = model/rating/BasicMF.py:9-26 (config #1),
 * 1 = model/rating/PMF.py:9-28 (regU, regI), 2 = model/rating/SVD.py:13-35 (biases d_Bu/d_Bi of the
 * tables' dtype, regB, global mean), 3 = model/rating/EE.py:15-34 (Euclidean embedding; *d_loss then also
 * carries the per-rating regU*|P[u]-Q[i]|^2 term of EE.py:25), 4 = model/rating/SocialMF.py:14-24 (PMF's arithmetic on
 * copies of P[u], Q[i]: the Q[i] update sees the old P[u]).  Rows are visited in array order (the caller passes the current
 * trainingData order); *d_loss receives sum(error^2).                                          */
int qrec_mf_sgd_ordered(void *d_P, void *d_Q, int dtype, int32_t d, int32_t ld,
                        const int32_t *d_u, const int32_t *d_i, const double *d_rating, int64_t n,
                        double lr, double *d_loss, int variant, double regU, double regI, void *d_Bu,
                        void *d_Bi, double regB, double global_mean, void *stream);

/* model/rating/SVDPlusPlus.py:25-62,70-86, order-exact: the implicit-feedback table d_Y [n_items][ld] next to P, Q and
 * the biases; d_rated_indptr/d_rated_items = each user's train items in data.userRated order (CSR over all users).
 * *d_loss receives sum(error^2); the epoch-end regularisers (:64-65) are qrec_sumsq.                        */
int qrec_svdpp_sgd_ordered(void *d_P, void *d_Q, void *d_Y, void *d_Bu, void *d_Bi, int dtype, int32_t d, int32_t ld,
                           const int64_t *d_rated_indptr, const int32_t *d_rated_items, const int32_t *d_u,
                           const int32_t *d_i, const double *d_rating, int64_t n, double lr, double regU, double regI,
                           double regB, double regY, double global_mean, double *d_loss, void *stream);

/* sum(x*x) over rows x d of a table (epoch-end regulariser, BPR.py:40); *d_out
 * (double) is overwritten. */
int qrec_sumsq(const void *d_x, int dtype, int64_t rows, int32_t d, int32_t ld, double *d_out,
               void *stream);

/* ---- graph recommenders (LightGCN family), TF-1.14 op semantics ----------------------- */

/* tf.sparse_tensor_dense_matmul(norm_adj, X) (model/ranking/LightGCN.py:17, NGCF.py:28,
 * SimGCL.py:25,33):  Y = A X  [+ addend_scale * addend]  and, if d_accum, accum += Y (the
 * running layer sum of LightGCN.py:19).  A is CSR (d_indices/d_values) cut by the host into
 * SEGMENTS of at most a few hundred non-zeros so that heavy rows do not serialise:
 * segment s covers non-zeros [seg_beg, seg_beg+seg_len) of row seg_row; seg_slot < 0 means
 * "the whole row, write Y directly", otherwise the partial sum goes to scratch slot
 * seg_slot of d_partial and long row k (long_row[k]) is the in-order sum of its
 * long_count[k] slots starting at long_first[k].  X, Y, addend, accum: [rows][ld] fp32,
 * ld in {32,64,128,256}.  Deterministic (no float atomics).  d_x_row_mask (may be NULL):
 * bitmap, bit c set iff row c of X is non-zero; clear rows are skipped (bit-identical result,
 * less traffic) -- used for the first backward SpMM, whose operand is the sparse batch gradient.
 * d_y_row_mask (may be NULL): bitmap of the OUTPUT rows that are wanted; the others are neither computed nor
 * written (Y, accum keep what they held) -- the last propagation layer of a training step is only read at the
 * batch's rows (embedding_lookup, LightGCN.py:22-24; qrec_mark_batch_rows builds the bitmap).
 * d_accum_init (may be NULL; needs d_accum): accum = accum_init + Y instead of accum += Y -- the first layer starts the
 * layer sum from the input table (LightGCN.py:15-19: all_embeddings = [ego_embeddings]), no copy before it.
 * d_addend_row_mask (may be NULL; needs d_addend): bitmap of the rows at which the addend is defined; elsewhere it counts as
 * zero and is not read -- the addend of the backward recurrences is the batch gradient, non-zero at the batch's rows only. */
int qrec_spmm_csr(const int32_t *d_seg_row, const int64_t *d_seg_beg, const int32_t *d_seg_len,
                  const int32_t *d_seg_slot, int64_t n_segs, const int32_t *d_long_row,
                  const int32_t *d_long_first, const int32_t *d_long_count, int32_t n_long,
                  const int32_t *d_indices, const float *d_values, const float *d_X, float *d_Y,
                  float *d_partial, int32_t ld, const float *d_addend, float addend_scale, float *d_accum,
                  const float *d_accum_init, const uint32_t *d_x_row_mask, const uint32_t *d_y_row_mask,
                  const uint32_t *d_addend_row_mask, void *stream);
/* d_row_mask |= bits of rows u[b], n_users+i[b], n_users+j[b] (bitmap over the joint [U;V] row space; clear it first) */
int qrec_mark_batch_rows(const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int32_t B, int32_t n_users,
                         uint32_t *d_row_mask, void *stream);

/* embedding_lookup x3 + util/loss.py:3-6 bpr_loss + the batch l2 term and all their gradients
 * (LightGCN.py:22-30): rows are S[row]/div (div = n_layers+1 folds the layer mean in), users
 * at rows [0,n_users), items at n_users+id.  dE (pre-zeroed, [n_rows][ld]) receives the
 * scatter-added row gradients; *d_loss (double) is ACCUMULATED into.  d_row_mask (may be NULL;
 * pre-zeroed, (n_rows+31)/32 words): bit r is set for every row of dE that receives a gradient.
 * d_ordered_ws (may be NULL): NULL = the row gradients are added with float atomics (throughput mode: right to fp32
 * rounding, summation order differs from launch to launch); a workspace of qrec_ordered_scatter_workspace_bytes(3 B, ld)
 * bytes = parity mode: every row's gradient is the sum of its lookups' slots in batch order, one lookup (u, i, j) at a
 * time -- the order of the reference's CPU scatter (UnsortedSegmentSum per IndexedSlices) -- same bits on every launch. */
int qrec_bpr_batch_loss_grad(const float *d_S, float div, int32_t n_users, int64_t n_rows, int32_t ld,
                             const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int32_t B, float eps,
                             float reg, float *d_dE, double *d_loss, uint32_t *d_row_mask, void *d_ordered_ws,
                             int64_t ordered_ws_bytes, void *stream);

/* Ordered scatter-add of rows (csrc/ordered.hip), the deterministic form of the gradient of tf.nn.embedding_lookup
 * (LightGCN.py:22-24, BUIR.py:88-95, SEPT.py:239; TF's UnsortedSegmentSum walks the slots in order on the CPU):
 *   d_out[d_dst_rows[s]] += sum of d_src[s][.] over the slots s with that destination, ascending s, class by class
 *   (class = s / class_size, the classes' sums added in class order; class_size 0 = one class); rows < 0 are skipped.
 * One stable rocPRIM radix sort of (row, slot) + one walk per run; fp32 adds in exactly that order, no contraction:
 * the result equals numpy's np.add.at(out, rows, src) bit for bit when out starts at zero.
 * Workspace: qrec_ordered_scatter_workspace_bytes(n_slots, ld) (also the size the d_ordered_ws arguments of
 * qrec_bpr_batch_loss_grad / qrec_buir_batch_loss_grad / qrec_sept_ssl_loss_grad take: 3 B, 2 B, n k slots). */
int qrec_ordered_scatter_workspace_bytes(int64_t n_slots, int32_t ld, int64_t *bytes);
int qrec_scatter_add_rows_ordered(const float *d_src, const int32_t *d_dst_rows, int64_t n_slots, int32_t ld, int64_t class_size,
                                  float *d_out, void *d_workspace, int64_t workspace_bytes, void *stream);

/* tf.train.AdamOptimizer dense update (LightGCN.py:31-32) in TF 1.14's ApplyAdam form, fp32,
 * with g = grad_scale * d_grad + grad_l2 * theta (grad_l2 = reg folds in d/dtheta of
 * reg*tf.nn.l2_loss(theta), model/ranking/BPR.py:83):  m += (g-m)(1-beta1); v += (g*g-v)(1-beta2);
 * theta -= (m*alpha)/(sqrt(v)+eps).  alpha = lr*sqrt(1-beta2^t)/(1-beta1^t) is supplied by
 * the host, which keeps the fp32 beta powers like TF does.                               */
int qrec_adam_step(float *d_theta, float *d_m, float *d_v, const float *d_grad, int64_t n_elems, float grad_scale,
                   float grad_l2, float alpha, float beta1, float beta2, float eps, void *stream);

/* ---- SimGCL (model/ranking/SimGCL.py) ---------------------------------------------------- */

/* perturbed_LightGCN_encoder's noise step (SimGCL.py:33-35) on one layer output: with x = d_src (or d_emb itself
 * when d_src is NULL: in place)  emb = x + sign(x) * l2_normalize(noise, axis=1) * eps, then (if d_accum) accum += emb.
 * The out-of-place form lets the two perturbed encoders share the first product A E with the clean one.
 * d_noise = [n_rows][ld] U[0,1) numbers, or NULL to draw them on the device with
 * Philox4x32-10(key=seed, counter={row, lane, stream_id}) -- same distribution as
 * tf.random.uniform, not TF's stream.
 * Injected noise may carry the sign to use in place of sign(x) (parity tests that follow a recorded run of the
 * reference: sign() is discontinuous at 0, so an entry of x within rounding of zero can take the other sign here
 * than it did there): a value v in [0, 1) is plain noise; +-(2 + u), u in [0, 1): noise u with the sign forced to
 * +-1; 4 + u: noise u with the sign forced to 0.  The l2_normalize of the row uses u.          */
int qrec_perturb_rows(float *d_emb, const float *d_src, int64_t n_rows, int32_t d, int32_t ld, float eps,
                      const float *d_noise, uint64_t seed, uint64_t stream_id, float *d_accum, const int32_t *d_row_ids,
                      const int32_t *d_n_row_ids, int32_t max_row_ids, int64_t philox_row0, void *stream);
/* The FIRST layer of SimGCL's three encoders in one pass (they share the product A E, SimGCL.py:23-36): emb_v = the
 * perturbed d_src (v = 1, 2: own noise / Philox stream each), and the three layer sums START here -- sum_v = emb_v,
 * src_sum = d_src (assigned, not accumulated: no zero-fill of the sums).  Row subset as for the NGCF calls below
 * (d_row_ids may be NULL): the last layer of a training step is read at the batch's rows only.  philox_row0 (both
 * calls): row r of these tables is row philox_row0 + r of the whole model (a rank's block of row-partitioned tables);
 * the Philox draws are keyed by that row. */
int qrec_perturb_two_views(const float *d_src, float *d_emb1, float *d_emb2, int64_t n_rows, int32_t d, int32_t ld, float eps,
                           const float *d_noise1, const float *d_noise2, uint64_t seed, uint64_t stream_id1, uint64_t stream_id2,
                           float *d_sum1, float *d_sum2, float *d_src_sum, const int32_t *d_row_ids, const int32_t *d_n_row_ids,
                           int32_t max_row_ids, int64_t philox_row0, void *stream);

/* One side (users or items) of SimGCL.calc_cl_loss (SimGCL.py:60-90) with its gradients.
 * x1 = S1[rows]/div, x2 = S2[rows]/div (the two perturbed views' rows of the batch's UNIQUE
 * nodes, n <= 16384, ids distinct); z = l2_normalize(x); loss = -sum log(exp(z1.z2/tau) /
 * sum_cols exp(z1 z2^T/tau)).  *d_loss (double) += loss (unscaled); d_out[rows] += cl_rate *
 * (dloss/dx1 + dloss/dx2), or, when d_out2 is given (SGL: the two views have different backward
 * operators, model/ranking/SGL.py:192-217), d_out += cl_rate*dloss/dx1 and d_out2 += cl_rate*dloss/dx2.
 * The n x n block runs on the f32 MFMA.                                                   */
int qrec_info_nce_workspace_bytes(int32_t n, int32_t ld, int64_t *bytes);
int qrec_info_nce_loss_grad(const float *d_S1, const float *d_S2, float div, const int32_t *d_rows, int32_t n,
                            int32_t ld, float tau, float cl_rate, void *d_workspace, float *d_out, float *d_out2,
                            double *d_loss, void *stream);

/* ---- NGCF dense layers (model/ranking/NGCF.py:27-42) ------------------------------------ *
 * Tables [rows][ld] fp32, ld in {32,64,128}; weights zero-padded to [ld][ld].             */

/* ROW SUBSETS.  The last layer of a TRAINING step is only read at the batch's rows (embedding_lookup, NGCF.py:44-46)
 * and its backward is zero everywhere else, so the three calls below take an optional ascending row list
 * d_row_ids[0 .. *d_n_row_ids) (device memory, built by qrec_compact_marked_rows; max_row_ids = the host's upper
 * bound on the count, used for the launch geometry): only the listed rows are read, computed and written, and the
 * weight gradients sum over the listed rows only.  d_row_ids == NULL: all n_rows rows.  Needs ld <= 64 for the two
 * MFMA calls.  Rows are addressed by their table index either way (no compacted copies).                    */

/* rows[0 .. *d_count) = the rows whose bit is set in a row bitmap (qrec_mark_batch_rows), ascending; at most
 * `capacity` rows are written and counted. */
int qrec_compact_marked_rows(const uint32_t *d_row_mask, int64_t n_rows, int32_t *d_rows, int32_t *d_count, int32_t capacity,
                             void *stream);

/* The row bitmap of a batch (as memset + qrec_mark_batch_rows would leave it) AND its ascending row list in one launch
 * (tables up to 2^20 rows: the bitmap is built in LDS; larger tables take the three separate steps).  d_rows / d_count may
 * both be NULL (bitmap only).  d_zero8[0 .. n_zero8) (n_zero8 <= 64, may be 0): doubles cleared by the same launch -- the
 * step's loss accumulators, which would otherwise cost a memset launch of their own. */
int qrec_mark_compact_batch_rows(const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int32_t B, int32_t n_users,
                                 int64_t n_rows, uint32_t *d_row_mask, int32_t *d_rows, int32_t *d_count, int32_t capacity,
                                 double *d_zero8, int32_t n_zero8, void *stream);

/* tf.unique of EVERY batch of an epoch's id stream (SimGCL.py:61-64), one launch: for batch b = ids[b*batch .. ) the
 * distinct ids in [0, id_range) (id_range <= 2^20), ascending, + out_offset, go to d_rows[b*batch ..) and their number to
 * d_counts[b].  Ascending instead of tf.unique's first-appearance order: the consumers (InfoNCE sums) are order-free. */
int qrec_unique_per_batch(const int32_t *d_ids, int64_t n, int32_t batch, int32_t id_range, int32_t out_offset, int32_t *d_rows,
                          int32_t *d_counts, void *stream);

/* pre = (side + E) W1 + (E * side) W2   (NGCF.py:29-31; side = A E from qrec_spmm_csr). f32 MFMA. */
int qrec_ngcf_dense_fwd(const float *d_E, const float *d_side, const float *d_W1, const float *d_W2, int64_t n_rows,
                        int32_t ld, float *d_pre, const int32_t *d_row_ids, const int32_t *d_n_row_ids, int32_t max_row_ids,
                        void *stream);
/* In place on d_pre_gate (in: pre, out: backward gate): nxt = dropout(leaky_relu(pre, 0.2), keep)
 * (NGCF.py:32-38; keep = 1 for the inference graph; d_mask = injected 0/1 keep decisions or NULL
 * for device Philox draws), z = l2_normalize(nxt) written to columns [col_off, col_off+d) of the
 * wide table (the concat of NGCF.py:42), 1/|nxt| to d_inv_norm.  philox_row0: row r of these tables is row
 * philox_row0 + r of the whole model (a rank's block of row-partitioned tables): the Philox draws are keyed by that row,
 * so a partitioned run drops the same entries as the single-GPU run.                      */
int qrec_ngcf_activate(float *d_pre_gate, int64_t n_rows, int32_t d, int32_t ld, float keep, const float *d_mask,
                       uint64_t seed, uint64_t stream_id, float *d_next, float *d_wide, int32_t wide_ld,
                       int32_t col_off, float *d_inv_norm, const int32_t *d_row_ids, const int32_t *d_n_row_ids,
                       int32_t max_row_ids, int64_t philox_row0, void *stream);
/* Backward of one layer: dnxt = dE_next (may be NULL) + normalize_bwd(dWide block); dpre = dnxt*gate;
 * dside = dpre W1^T + (dpre W2^T)*E ; dE = dpre W1^T + (dpre W2^T)*side (caller adds A^T dside);
 * gW1 = (side+E)^T dpre, gW2 = (E*side)^T dpre (deterministic two-stage reduction over nodes).
 * With a row subset d_dpre / d_dside / d_dE are written at the listed rows only (the caller zero-fills what it reads
 * elsewhere); d_partial must hold qrec_ngcf_wgrad_partial_bytes(n_rows, ld) bytes either way.
 * d_wide_row_mask (may be NULL): row bitmap of the rows at which d_dWide is defined (the batch's rows, cleared with
 * qrec_zero_rows before the loss scatter instead of zero-filling the whole wide table); elsewhere its block counts as 0. */
int qrec_ngcf_layer_bwd(const float *d_dE_next, const float *d_dWide, const float *d_wide, int32_t wide_ld,
                        int32_t col_off, const float *d_inv_norm, const float *d_gate, const float *d_E,
                        const float *d_side, const float *d_W1, const float *d_W2, int64_t n_rows, int32_t d,
                        int32_t ld, float *d_dpre, float *d_dside, float *d_dE, float *d_partial, float *d_gW1,
                        float *d_gW2, const int32_t *d_row_ids, const int32_t *d_n_row_ids, int32_t max_row_ids,
                        const uint32_t *d_wide_row_mask, void *stream);
int qrec_ngcf_wgrad_partial_bytes(int64_t n_rows, int32_t ld, int64_t *bytes);
/* dst[row][c] (=|+=) src[row][src_col_off + c], c < d : moves the ego block in and out of the wide table; with a row
 * subset (see above) only the listed rows are touched. */
int qrec_copy_cols(float *d_dst, int32_t dst_ld, const float *d_src, int32_t src_ld, int32_t src_col_off, int64_t n_rows,
                   int32_t d, int32_t accumulate, const int32_t *d_row_ids, const int32_t *d_n_row_ids, int32_t max_row_ids,
                   void *stream);
/* X[row][0 .. ld) = 0 for the listed rows (a row subset as above): clears a gradient table where the next scatter lands */
int qrec_zero_rows(float *d_X, int32_t ld, const int32_t *d_row_ids, const int32_t *d_n_row_ids, int32_t max_row_ids, void *stream);

/* ---- the dense layer of DiffNet / DHCF (model/ranking/DiffNet.py:46-49, DHCF.py:74-87; csrc/dense_layer.hip) ---- *
 * Tables [n_rows][ld] fp32, ld in {32, 64, 128} (anything else is refused).  d_W holds one zero-padded [ld][ld] block per
 * operand: block 0 multiplies X1, block 1 multiplies X2 (a (2d x d) weight = its two d x d halves).  No float atomics:
 * the same inputs give the same bits on every launch.                                                          */

/* Y = [X1 | X2] W (+ R), through ReLU when relu != 0.  d_X2 and d_R may be NULL. */
int qrec_dense_layer_fwd(const float *d_X1, const float *d_X2, const float *d_W, const float *d_R, int64_t n_rows, int32_t ld,
                         int32_t relu, float *d_Y, void *stream);
/* ReluGrad: dpre = dY where Y > 0, else 0 */
int qrec_dense_layer_dpre_relu(const float *d_dY, const float *d_Y, int64_t n_rows, int32_t ld, float *d_dpre, void *stream);
/* Backward of qrec_ngcf_activate when the NORMALISED rows are what the next layer carries on (DHCF.py:78-90):
 * dz = block [col_off, col_off + d) of d_dWide + d_dZ_next (may be NULL); dpre = (dz - z (z.dz)) * inv_norm * gate. */
int qrec_dense_layer_dpre_norm(const float *d_dWide, const float *d_wide, int32_t wide_ld, int32_t col_off, const float *d_dZ_next,
                               const float *d_inv_norm, const float *d_gate, int64_t n_rows, int32_t d, int32_t ld, float *d_dpre,
                               void *stream);
/* dX1 (+= when accumulate_dX1, else =) dpre W[0]^T; dX2 = dpre W[1]^T; gW[w] = X_w^T dpre (per-slab partial products in
 * d_ws, added in slab order).  The residual's gradient is dpre itself.  d_X2 / d_dX2 both NULL or both given.
 * d_ws: at least qrec_dense_layer_ws_bytes(n_rows, ld, n_w) bytes, n_w = 1 or 2 operands; a smaller one is refused. */
int qrec_dense_layer_bwd(const float *d_dpre, const float *d_X1, const float *d_X2, const float *d_W, int64_t n_rows, int32_t ld,
                         int32_t accumulate_dX1, float *d_dX1, float *d_dX2, float *d_gW, void *d_ws, int64_t ws_bytes,
                         void *stream);
int qrec_dense_layer_ws_bytes(int64_t n_rows, int32_t ld, int32_t n_w, int64_t *bytes);
/* The loss of qrec_bpr_batch_loss_grad (same rows, same per-triplet arithmetic) in a FIXED order, for parity runs: that call adds
 * its blocks' sums with fp64 atomics, whose order -- and with it the last bits of the loss -- changes from launch to launch.
 * Block k of n_slots walks its triplets in order and ASSIGNS its sum to d_slots[k]; the loss is the slots added in order
 * (host).  No gradient is formed here. */
int qrec_bpr_batch_loss_slots(const float *d_S, float div, int32_t n_users, int32_t ld, const int32_t *d_u, const int32_t *d_i,
                              const int32_t *d_j, int32_t B, float eps, float reg, double *d_slots, int32_t n_slots, void *stream);

/* ---- per-epoch graph augmentation on the device (SGL.py:113-155, BUIR.py:41-65; throughput mode) ----------------------------
 * A sub-graph of the training graph as a VALUE array over the full graph's CSR structure (csrc/augment.hip): entry e of the joint
 * adjacency gets fl32(fl32(d'_r a'_e) d'_c) with a'_e = the number of kept training rows that map to it and d' = deg'^-1/2 of the
 * kept edges (0 for isolated nodes), dropped entries 0 -- the reference's re-normalised sub-adjacency, laid out for the SpMM plan
 * that already exists.  d_u / d_i: the training rows (user id, item id), d_pos_ui / d_pos_iu: the CSR positions of a row's two
 * entries (u, U + i) and (U + i, u); d_row_of_nnz / d_indices: row and column of every CSR entry; d_dinv_table[k] = float32
 * power(k, -0.5) for k = 0 .. max_deg (inf -> 0; formed by the host with numpy, so the values carry the reference's bits).
 * The draw is the caller's (qrec_random_permutations): d_keep_rows = n_keep kept training rows (edge dropout, random walk) OR
 * d_drop_users / d_drop_items = dropped node ids (node dropout; d_flags: n_users + n_items bytes of scratch) OR neither (the full
 * graph).  Scratch: d_cnt int32[nnz], d_deg int32[n_users + n_items].  Integer atomics only: the result is deterministic. */
int qrec_subgraph_values(const int32_t *d_u, const int32_t *d_i, const int32_t *d_pos_ui, const int32_t *d_pos_iu, int64_t n_edges,
                         int32_t n_users, int32_t n_items, const int32_t *d_keep_rows, int64_t n_keep, const int32_t *d_drop_users,
                         int64_t n_drop_users, const int32_t *d_drop_items, int64_t n_drop_items, const int32_t *d_row_of_nnz,
                         const int32_t *d_indices, int64_t nnz, const float *d_dinv_table, int32_t max_deg, int32_t *d_cnt,
                         int32_t *d_deg, uint8_t *d_flags, float *d_values, void *stream);

/* SEPT's per-epoch perturbed joint graph (model/ranking/SEPT.py:84-111, get_adj_mat(is_subgraph=True)) as two value arrays over a fixed
 * structure: the sorted CSR pattern of R + R^T + F over the n_users + n_items nodes (R: the training rows, F: the pruned follow pairs at
 * (follower, followee) only), which holds the non-zeros of every epoch's graph.  d_pos_ui / d_pos_iu [n_edges]: the CSR positions of a
 * training row's two entries; d_pos_f [n_pairs]: the position of a follow pair's entry; d_keep_rows / d_keep_pairs: the kept rows and pairs
 * (prefixes of the caller's permutations; duplicated rows and pairs add up).  d_keep_rows == NULL keeps every training row and
 * d_keep_pairs == NULL (with n_keep_pairs == 0) no pair: the plain joint adjacency the reference returns for drop_rate <= 0 (:98-103).
 * d_indptr [n + 1], d_row_of_nnz / d_indices [nnz]: the structure; d_pos_t [nnz]: where entry e sits in the CSR of the TRANSPOSED structure.
 * An entry's weight a is its count in the rating blocks and count^2 in the user-user block; a node's degree is the sum of the weights of
 * its ROW; value = fl32(fl32(dinv[deg_row] a) dinv[deg_col]), 0 for entries nothing was kept of, with d_dinv_table[k] = float32
 * power(k, -0.5) for k = 0 .. max_deg (inf -> 0; made by the host with numpy; max_deg >= the full graph's largest weighted row sum).
 * d_values [nnz]: M in the structure's order; d_values_t [nnz]: M^T in the transposed structure's order.  Scratch: d_cnt int32[nnz],
 * d_deg int32[n_users + n_items].  Integer atomics only: bit-identical to the reference's scipy arithmetic, the same bits every run. */
int qrec_sept_perturbed_values(const int32_t *d_pos_ui, const int32_t *d_pos_iu, int64_t n_edges, const int32_t *d_pos_f, int64_t n_pairs,
                               const int32_t *d_keep_rows, int64_t n_keep_rows, const int32_t *d_keep_pairs, int64_t n_keep_pairs,
                               int32_t n_users, int32_t n_items, const int64_t *d_indptr, const int32_t *d_row_of_nnz,
                               const int32_t *d_indices, const int32_t *d_pos_t, int64_t nnz, const float *d_dinv_table, int32_t max_deg,
                               int32_t *d_cnt, int32_t *d_deg, float *d_values, float *d_values_t, void *stream);

/* ---- BUIR (model/ranking/BUIR.py) ------------------------------------------------------------------ *
 * The propagation of both encoders is qrec_spmm_csr on the epoch's two sub-graphs.  What the model adds:      */

/* Per batch element b (u = d_u[b], i = n_users + d_i[b]), with x = S_online[row]/div, t = S_target[row]/div
 * (div = n_layers + 1 folds the layer mean in): q = tanh(x W + bias) (BUIR.py:105-107),
 * *d_loss += [(1 - cos(q_u, t_i)) + (1 - cos(q_i, t_u))] / 2 (:127-129, tf.math.l2_normalize eps 1e-12), the gradient
 * w.r.t. the online mean rows is scatter-added into d_dS (un-divided: the caller folds 1/div into its optimizer
 * step), and the (x, dpre) pairs go to d_X / d_dPre rows b (user side) and B + b (item side) for qrec_buir_wgrad.
 * d_W [ld][ld], d_bias [ld], zero-padded; tables [rows][ld], ld in {32, 64, 128}.
 * d_ordered_ws (nullable, qrec_ordered_scatter_workspace_bytes(2 B, ld)): parity mode -- the scatter into d_dS adds each
 * row's slots in batch order instead of with float atomics (see qrec_bpr_batch_loss_grad).                */
int qrec_buir_batch_loss_grad(const float *d_S_online, const float *d_S_target, float div, int32_t n_users, int32_t ld,
                              const float *d_W, const float *d_bias, const int32_t *d_u, const int32_t *d_i, int32_t B,
                              float *d_dS, float *d_X, float *d_dPre, double *d_loss, void *d_ordered_ws, int64_t ordered_ws_bytes,
                              void *stream);
/* d_gW = X^T dPre, d_gb = column sums of dPre over n_rows (= 2B) pairs; deterministic two-stage sum through
 * d_scratch (qrec_buir_wgrad_scratch_bytes).                                                              */
int qrec_buir_wgrad_scratch_bytes(int32_t ld, int64_t *bytes);
int qrec_buir_wgrad(const float *d_X, const float *d_dPre, int32_t n_rows, int32_t ld, float *d_scratch, float *d_gW,
                    float *d_gb, void *stream);
/* target = target*tau + online*(1 - tau) (BUIR.py:120-123, run after every optimizer step :159)           */
int qrec_ema_update(float *d_target, const float *d_online, float tau, int64_t n_elems, void *stream);

/* ---- full-rank evaluation: base/recommender.py:143-150 + util/qmath.py:134-146 -------- *
 * For each of the n_batch_users users (ids into the user table): scores = V . U[user]
 * (MFMA), scores of the user's rated train items set to 0 (rated CSR over ALL users, may be
 * NULL), then the reference's find_k_largest: min-heap of (score,id) seeded with the first
 * N items, strict '>' replacement, stable descending sort -- ties included, so ids are
 * bit-identical to the reference's.  Outputs [n_batch_users][N] (ids -1 padded when
 * n_items < N).  Tables are [rows][ld] with ld a multiple of 32 floats / 16 doubles and columns [d, ld) zero.
 * N <= 100 as in base/recommender.py:132-134.  Two routes, same lists:
 *   fused (fp32, ld <= 128, N <= 63, n_items >= 16,384): a per-user threshold, then a pass that keeps only the items
 *     whose score reaches it -- no users x items block is ever written.  For ld = 32 / 64 / 128 both passes run on bf16
 *     copies of the tables (v_mfma_f32_32x32x16_bf16) against thresholds lowered by a proven bound on the rounding, and the
 *     few dozen survivors per user are re-scored by the block route's own fp32 MFMA sequence, so ids and scores are
 *     bit-identical to the block route's (env QREC_EVAL_F32_FILTER: both passes in fp32, as for other ld).  Users whose
 *     N+1 best scores are not pairwise distinct (the only case in which the heap's history shows) get the exact
 *     sequential walk, a few hundred at a time.  The rated CSR must then have ASCENDING item ids inside a row.  The call
 *     synchronises `stream` once (it reads back how many such users there are).
 *   block (everything else; forced by env QREC_EVAL_BLOCK_PATH): scores into a transposed users x items block in
 *     d_scratch, mask, sliced top-N with exact fallbacks.
 * Size d_scratch with qrec_score_topk_scratch_bytes (same dtype / sizes / ld / N).                                  */
int qrec_score_topk_scratch_bytes(int dtype, int32_t n_items, int32_t n_batch_users, int32_t ld, int32_t N, int64_t *bytes);
int qrec_score_topk(const void *d_U, const void *d_V, int dtype, int32_t d, int32_t ld, int32_t n_items,
                    const int32_t *d_user_ids, int32_t n_batch_users, const int64_t *d_rated_indptr,
                    const int32_t *d_rated_items, int32_t N, void *d_scratch, int32_t *d_ids_out,
                    void *d_scores_out, void *stream);

/* Measure.hits (util/measure.py:15-21) + the DCG sum of Measure.NDCG (util/measure.py:70-82) over the lists of a
 * previous qrec_score_topk, still on the device: for batch row b (user d_user_ids[b]) and its first n_cut ids,
 * d_hits_out[b] = how many are among the user's test items (CSR over ALL users, item ids ascending inside a
 * row, items unknown to the training set left out), d_dcg_out[b] = sum of d_discount[pos] over the hit
 * positions, added in rank order.  The caller passes discount[pos] = 1/log(pos+2) as ITS doubles, so the
 * per-user values -- and the Precision/Recall/NDCG strings built from them -- equal the reference's bit for bit. */
int qrec_rank_hits(const int32_t *d_ids, int32_t n_batch_users, int32_t row_stride, int32_t n_cut,
                   const int32_t *d_user_ids, const int64_t *d_test_indptr, const int32_t *d_test_items,
                   const double *d_discount, int32_t *d_hits_out, double *d_dcg_out, void *stream);

/* ---- the on-disk rating format: util/io.py:31-76 (FileIO.loadDataSet) --------------------------- *
 * "user item rating" text, one record per line, fields split on every single character of `delims`
 * (NULL = the reference's " ,\t"), columns picked by index (col_rating < 0: no rating column, rating = 1),
 * skip_header drops the first line, binarize drops records rated below `threshold` and sets the rest to 1.
 * The result holds dense ids in first-appearance order, the ratings and the '\n'-joined name tables
 * (which: 0 = users, 1 = items).  Host code, no GPU.  QREC_ERR_UNSUPPORTED = the file needs CPython's own
 * parsing rules (non-ASCII text, exotic float literals, short records): the caller then runs the Python path. */
typedef struct qrec_ratings qrec_ratings;
int qrec_ratings_load(const char *path, const char *delims, int32_t col_user, int32_t col_item, int32_t col_rating,
                      int32_t skip_header, int32_t binarize, double threshold, qrec_ratings **out);
int64_t qrec_ratings_rows(const qrec_ratings *h);
int32_t qrec_ratings_count(const qrec_ratings *h, int32_t which);
int64_t qrec_ratings_names_bytes(const qrec_ratings *h, int32_t which);
int qrec_ratings_copy(const qrec_ratings *h, int32_t *user_out, int32_t *item_out, double *rating_out);
int qrec_ratings_names(const qrec_ratings *h, int32_t which, char *out);
void qrec_ratings_free(qrec_ratings *h);

/* ---- SEPT (model/ranking/SEPT.py): per-layer normalised views, pseudo labels, several-positives contrastive loss ----
 * qrec_l2norm_rows_accum: inv[r] = rsqrt(max(|X[r]|^2, 1e-12)), S[r] += X[r] * inv[r]  -- one propagated layer entering a
 *   view's sum as tf.math.l2_normalize(x, axis=1) (SEPT.py:144-160).  qrec_l2norm_rows_bwd: its gradient w.r.t. X[r],
 *   out[r] = (dS[r] - z (z . dS[r])) * inv[r], z = X[r] * inv[r] (autodiff of the same lines).  qrec_scale_copy:
 *   dst = alpha * src (the Variable / 2 of SEPT.py:129-130).  ld in {32, 64, 128, 256} floats, rows zero-padded. */
int qrec_l2norm_rows_accum(const float *d_X, int64_t n_rows, int32_t ld, float *d_S, float *d_inv, void *stream);
int qrec_l2norm_rows_bwd(const float *d_X, const float *d_inv, const float *d_dS, int64_t n_rows, int32_t ld, float *d_out,
                         void *stream);
int qrec_scale_copy(float *d_dst, const float *d_src, int64_t n_elems, float alpha, void *stream);
/* qrec_sept_ssl_loss_grad: label_prediction + generate_pesudo_labels + neighbor_discrimination (SEPT.py:214-262) on the
 *   n distinct users of a batch (d_rows, tf.unique order).  z_v = l2_normalize(S_v[rows]) for the friend / sharing /
 *   preference views, a = l2_normalize(S_aug[rows]); prob_v = softmax(z_v a^T); labels_v = top_k of the OTHER two
 *   encoders' averaged prob (k = ins_cnt, equal scores in index order);
 *   loss += -sum_i log( sum_{l in labels_v[i]} e^{z_v[i].a[l]/0.1} / sum_j e^{z_v[i].a[j]/0.1} ) over the three encoders
 *   (UNSCALED, added to *d_loss); dS_v[rows[i]] += ss_rate * d loss / d S_v[rows[i]] for the four tables.
 *   d_labels (nullable): int32 [3][n][k] pseudo labels (positions in d_rows) for inspection.
 *   d_ordered_ws (nullable, qrec_ordered_scatter_workspace_bytes(n k, ld)): parity mode -- the positives' part of the augmented
 *   view's gradient (rows shared by several users' label sets) is added per row in (user, label) order instead of with float atomics. */
int qrec_sept_ssl_workspace_bytes(int32_t n, int32_t ld, int32_t k, int64_t *bytes);
int qrec_sept_ssl_loss_grad(const float *d_S_friend, const float *d_S_sharing, const float *d_S_pref, const float *d_S_aug,
                            const int32_t *d_rows, int32_t n, int32_t ld, int32_t k, float ss_rate, void *d_workspace,
                            float *d_dS_friend, float *d_dS_sharing, float *d_dS_pref, float *d_dS_aug, double *d_loss,
                            int32_t *d_labels, void *d_ordered_ws, int64_t ordered_ws_bytes, void *stream);

/* ---- TBPR: model/ranking/TBPR.py (numpy path) -----------------------------------------------------------------
 * qrec_mt_tbpr_sample_epoch (host): the sampling loop TBPR.py:131-158 on the CPython MT19937 stream -- per user and
 *   positive item the chain [i, choice(joint)?, choice(weak)?, choice(strong)?, k] (k: random item, redrawn while
 *   positive); writes the (u, a, b) updates of consecutive chain members.  The three item lists are CSR over users.
 * qrec_tbpr_sgd_ordered: TBPR.optimization (TBPR.py:40-48) over those triplets strictly in order (a == b occurs and is
 *   applied as two sequential updates of one row), d_loss2[0] = sum(-log s), d_loss2[1] = sum over users of
 *   regU*sum(P*P) + regI*sum(Q*Q) taken after each user's updates (TBPR.py:159); d_sums_in = {sum(P*P), sum(Q*Q)}
 *   of the tables at launch (qrec_sumsq).                                                                            */
int qrec_mt_tbpr_sample_epoch(uint32_t *state625, const int64_t *pos_indptr, const int32_t *pos_items, int32_t n_users,
                              int32_t n_items, const int64_t *joint_indptr, const int32_t *joint_items,
                              const int64_t *weak_indptr, const int32_t *weak_items, const int64_t *strong_indptr,
                              const int32_t *strong_items, int64_t capacity, int32_t *u_out, int32_t *a_out, int32_t *b_out,
                              int64_t *n_out);
int qrec_tbpr_sgd_ordered(void *d_P, void *d_Q, int dtype, int32_t d, int32_t ld, const int32_t *d_u, const int32_t *d_a,
                          const int32_t *d_b, int64_t n, double lr, double regU, double regI, const double *d_sums_in,
                          double *d_loss2, void *stream);

/* ---- SBPR: model/ranking/SBPR.py:31-78 (numpy path) ------------------------------------------------------------------
 * The reference's file raises TypeError at :46 (`self.FPSet[user][kItems]`, a dict indexed with a list) for the first user who has
 * social feedback; both entry points implement the loop with that subscript read as `item_k` and everything else as written
 * (tests/golden/gen_golden.py case_sbpr_filmtrust: the reference's own source with that one token replaced is the fixture).
 * qrec_mt_sbpr_sample_epoch (host): the draws of SBPR.py:37-55,69-72 on the CPython MT19937 stream -> rows (u, i, k or -1, j, Suk),
 *   int32 [n][5].  ps_users: user ids in PositiveSet's key order; fp_*: FPSet as CSR over user ids (items in dict order, counts);
 *   item_key_user[j]: id of the user whose NAME equals item j's name or -1, is_key[user] (in/out): that user is a key of the
 *   defaultdict FPSet by now -- the negative's rejection test `item_j in self.FPSet` (:52) is an item name looked up among user names.
 * qrec_sbpr_sgd_ordered: SBPR.py:41-74 over those rows strictly in order (rows with i < 0: a bare visit of a user without positives).
 *   d_bias: the item biases b [n_items] in the tables' dtype (never updated by the reference); bias_sumsq = b.b;
 *   d_loss2[0] = sum of the -log terms (:57-58, :73), d_loss2[1] = sum over users of regU*sum(P*P) + regI*sum(Q*Q) + b.b (:74);
 *   d_sums_in = {sum(P*P), sum(Q*Q)} of the tables at launch (qrec_sumsq).                                                       */
int qrec_mt_sbpr_sample_epoch(uint32_t *state625, const int32_t *ps_users, int32_t n_ps, const int64_t *pos_indptr, const int32_t *pos_items,
                              int32_t n_users, int32_t n_items, const int64_t *fp_indptr, const int32_t *fp_items, const int32_t *fp_counts,
                              const int32_t *item_key_user, uint8_t *is_key, int64_t capacity, int32_t *rows_out, int64_t *n_out);
int qrec_sbpr_sgd_ordered(void *d_P, void *d_Q, const void *d_bias, int dtype, int32_t d, int32_t ld, const int32_t *d_rows, int64_t n, double lr,
                          double regU, double regI, double bias_sumsq, const double *d_sums_in, double *d_loss2, void *stream);

/* ---- MHCN: model/ranking/MHCN.py:93-216 (self-gating, channel attention, hierarchical self-supervision) ---------------
 * Tables [rows][ld] fp32, ld in {32, 64, 128, 256}, columns >= d zero; d x d weights zero-padded to [ld][ld], biases [ld].
 * qrec_gate_fwd / _bwd serve ld in {32, 64, 128} only: they stage the whole [ld][ld] weight matrix in LDS, and 256 KiB at
 *   ld = 256 is more than a CU has.  Stride 256 is refused with a message; the attention and hss entry points keep it.
 * qrec_gate_fwd:  Y = X * sigmoid(X W + b), S = sigmoid(.)  -- self_gating / self_supervised_gating (MHCN.py:109-112).
 * qrec_gate_bwd:  Q = (dy_scale dY) * X * S (1 - S);  dX (+)= dy_scale dY * S + Q W^T.  The weight gradients are
 *   dW = X^T Q, db = column sums of Q: qrec_buir_wgrad(X, Q, ...).
 * qrec_channel_attention_fwd (MHCN.py:113-121): v = att_mat att^T (d_v, [ld] scratch kept for the backward pass),
 *   score = softmax_k(e_k . v) ([rows][4], 4th unused), out = sum_k score_k e_k + half / 2 (half nullable).
 * qrec_channel_attention_bwd: de_k (+)= score_k dOut + dw_k v (accumulate flag), dhalf (+)= dOut / 2 (nullable),
 *   g_att += att_mat^T dv, g_att_mat += dv (x) att with dv = sum_rows sum_k dw_k e_k (d_dv_scratch:
 *   qrec_channel_attention_scratch_bytes; the column sums dv, graph, d graph are formed in a fixed order -- per-block partials
 *   added in block order, no float atomics -- so the weight gradients have the same bits on every launch).
 * qrec_hss_loss_grad: hierarchical_self_supervision (MHCN.py:184-206) given edge = H em and the call's five shuffles
 *   (row p1; column k2 then row p2; column k3 then row p3 -- tf.random.shuffle of range(n) / range(d)) with their
 *   inverses: *d_loss += local + global MIM loss (unscaled); d_dem / d_dedge = scale * gradient w.r.t. em / edge
 *   (overwritten).  d_scratch: qrec_hss_scratch_bytes(n).
 * qrec_random_permutations: `count` uniformly random permutations of range(n) ([count][n]) and their inverses from ONE
 *   rocPRIM radix sort (key = permutation number << 40 | 40 Philox bits); qrec_small_permutations: `count` Fisher-Yates permutations of range(n <= 4096) with inverses. */
int qrec_gate_fwd(const float *d_X, const float *d_W, const float *d_bias, int64_t n_rows, int32_t ld, float *d_Y, float *d_S,
                  void *stream);
int qrec_gate_bwd(const float *d_X, const float *d_S, const float *d_dY, const float *d_W, int64_t n_rows, int32_t d, int32_t ld,
                  float dy_scale, float *d_Q, float *d_dX, int32_t accumulate, void *stream);
int qrec_channel_attention_fwd(const float *d_e1, const float *d_e2, const float *d_e3, const float *d_att, const float *d_att_mat,
                               const float *d_half, int64_t n_rows, int32_t ld, float *d_v, float *d_score, float *d_out,
                               void *stream);
int qrec_channel_attention_bwd(const float *d_dOut, const float *d_e1, const float *d_e2, const float *d_e3, const float *d_score,
                               const float *d_v, const float *d_att, const float *d_att_mat, int64_t n_rows, int32_t ld,
                               float *d_de1, float *d_de2, float *d_de3, int32_t accumulate, float *d_dhalf, int32_t half_accumulate,
                               float *d_dv_scratch, float *d_g_att, float *d_g_att_mat, void *stream);
int qrec_channel_attention_scratch_bytes(int64_t *bytes);
int qrec_hss_scratch_bytes(int64_t n_rows, int64_t *bytes);
int qrec_hss_loss_grad(const float *d_em, const float *d_edge, int64_t n_rows, int32_t d, int32_t ld, const int32_t *d_p1,
                       const int32_t *d_p1inv, const int32_t *d_p2, const int32_t *d_p2inv, const int32_t *d_k2,
                       const int32_t *d_k2inv, const int32_t *d_p3, const int32_t *d_p3inv, const int32_t *d_k3,
                       const int32_t *d_k3inv, float scale, float *d_scratch, float *d_dem, float *d_dedge, double *d_loss,
                       void *stream);
int qrec_random_permutations_scratch_bytes(int64_t n, int32_t count, int64_t *bytes);
int qrec_random_permutations(int64_t n, int32_t count, uint64_t seed, uint64_t stream_id, void *d_scratch, int32_t *d_perms,
                             int32_t *d_invs, void *stream);
int qrec_small_permutations(int32_t n, int32_t count, uint64_t seed, uint64_t stream_id, int32_t *d_perms, int32_t *d_invs,
                            void *stream);

/* ---- multi-GPU: collectives and the kernels around them ------------------------------------- *
 * The reference has no distributed code (its only parallelism is one process per CV fold, QRec.py:57-89); the
 * contract is BASELINE.json's north star: one process per GPU, embedding tables row-sharded, RCCL over xGMI.  librccl
 * is bound directly (dlopen'ed on first use from the directory of the HIP runtime this library runs on; QREC_RCCL_LIB
 * overrides) -- no torch tensor or torch kernel is involved.  Every collective only ENQUEUES on `stream`.
 *   qrec_comm_unique_id : rank 0 makes the 128-byte id, the launcher's control plane hands it to every rank;
 *   qrec_comm_init      : collective over all ranks, binds the device selected by qrec_init;
 *   qrec_allreduce      : in-place sum (QREC_F32 / QREC_F64 / QREC_I32);  _pair: two buffers, ONE fused launch (the
 *                         item-table deltas + the epoch's loss terms);
 *   qrec_allgather / qrec_reduce_scatter : `count` elements per rank (graph models: operand rows of a row-partitioned
 *                         propagation and the transposed product of its backward pass);
 *   qrec_alltoall_rows  : segment p of d_send (h_send_rows[p] rows of row_bytes, segments back to back in rank order)
 *                         goes to rank p, segment p of d_recv comes from rank p -- cross-shard row lookups and the
 *                         return of their updates.  Counts are HOST arrays of `world` entries.                       */
#define QREC_COMM_UID_BYTES 128
int qrec_comm_library(char *path_out, int path_len, int *version);
int qrec_comm_unique_id(uint8_t *h_uid);
int qrec_comm_init(int32_t world, int32_t rank, const uint8_t *h_uid, void **comm);
int qrec_comm_destroy(void *comm);
int qrec_comm_info(void *comm, int32_t *world, int32_t *rank);
/* what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): the ranks that really
 * joined, this process's rank among them and the HIP device it is bound to -- bench.py prints them next to a multi-GPU result */
int qrec_comm_query(void *comm, int32_t *rccl_ranks, int32_t *rccl_rank, int32_t *device);
int qrec_allreduce(void *comm, void *d_buf, int64_t count, int dtype, void *stream);
int qrec_allreduce_pair(void *comm, void *d_a, int64_t count_a, int dtype_a, void *d_b, int64_t count_b, int dtype_b,
                        void *stream);
int qrec_allgather(void *comm, const void *d_send, void *d_recv, int64_t count, int dtype, void *stream);
int qrec_reduce_scatter(void *comm, const void *d_send, void *d_recv, int64_t count, int dtype, void *stream);
int qrec_alltoall_rows(void *comm, const void *d_send, const int64_t *h_send_rows, void *d_recv,
                       const int64_t *h_recv_rows, int64_t row_bytes, void *stream);
/* One fused launch of arbitrary point-to-point segments: send k = h_send_bytes[k] bytes at d_send + h_send_off[k] to rank
 * h_send_peer[k]; receive k likewise.  Between two ranks sends and receives are matched in list order (both sides list a pair's
 * segments in the same order).  The row-sharded BPR layout ships the request ids of ALL batches of an epoch with it.       */
int qrec_sendrecv_segments(void *comm, const void *d_send, const int32_t *h_send_peer, const int64_t *h_send_off,
                           const int64_t *h_send_bytes, int32_t n_send, void *d_recv, const int32_t *h_recv_peer,
                           const int64_t *h_recv_off, const int64_t *h_recv_bytes, int32_t n_recv, void *stream);

/* Replicated item table (every rank trains its own users against a full copy of Q): after a step
 *     delta = Q - Q_start;  all-reduce(delta);  Q_start += delta;  Q = Q_start
 * so that every rank's updates are kept and the replicas stay bit-identical.  n = rows*ld floats (multiple of 4).     */
/* The same around the step's ONE collective, fused with the epoch's loss terms (fp32 tables; users sharded, items
 * replicated): qrec_dist_epoch_pre = { delta = Q - Q_start; d_stats[1] = sum P*P of this rank's users }, the caller
 * all-reduces {d_delta, d_stats[0..1]} (qrec_allreduce_pair), qrec_dist_epoch_post = { Q_start += delta; Q = Q_start;
 * d_stats[2] = sum Q*Q; the reference's epoch decision as in qrec_epoch_close }.  Sums are taken in block order:
 * every rank computes the same bits and takes the same decision.                                                    */
int qrec_dist_epoch_pre(const float *d_P, int64_t p_rows, int32_t ld, const float *d_Q, const float *d_Q_start,
                        float *d_delta, int64_t q_rows, double *d_stats, const double *d_state, void *stream);
int qrec_dist_epoch_post(float *d_Q, float *d_Q_start, const float *d_delta, int64_t q_rows, int32_t ld, double *d_stats,
                         double *d_state, double regU, double regI, double max_lr, double tol, double *d_log,
                         int64_t log_capacity, void *stream);
int qrec_table_delta(const float *d_table, const float *d_start, float *d_delta, int64_t n, void *stream);
int qrec_table_apply(float *d_table, float *d_start, const float *d_delta, int64_t n, void *stream);

/* Row-sharded item table: item id = r*world + o is local row r of rank o (interleaved, so that popular items spread
 * over the ranks).  qrec_shard_rows = rows a rank holds.
 * qrec_shard_plan_batch, for n triplets with global item ids d_i / d_j:
 *   d_req_rows : the DISTINCT items the batch touches as local rows at their owner, grouped by owner in rank order and
 *                ascending inside a group (capacity min(2n, n_items));  d_counts[world] = rows per owner;
 *   d_ci, d_cj : the triplets' item ids rewritten as positions in d_req_rows, i.e. rows of the batch's row cache.
 * Everything stays on the device; the caller reads d_counts back when it needs the sizes of the exchange.
 * qrec_shard_plan_epoch: the same plan for ALL n_batches batches of an epoch in one set of launches -- batch b = triplets
 *   [d_bounds[b], d_bounds[b + 1]) (device int64[n_batches + 1]), its request list at d_req_rows + d_req_off[b] (device
 *   int64[n_batches]), its counts at d_counts[b * world]; scratch: qrec_shard_plan_epoch_scratch_bytes.
 * qrec_gather_rows: d_out[k] = d_table[d_rows[k]] (an owner answering a request).
 * qrec_scatter_add_row_deltas: d_table[d_rows[k]] += d_fresh[k] - d_sent[k] with f32 atomics (an owner taking back the
 *   rows it lent: several ranks may return the same row, every rank's updates are kept).                             */
int qrec_shard_rows(int64_t n_items, int32_t world, int32_t rank, int64_t *rows);
int qrec_shard_plan_scratch_bytes(int64_t n_items, int32_t world, int64_t *bytes);
int qrec_shard_plan_batch(const int32_t *d_i, const int32_t *d_j, int64_t n, int64_t n_items, int32_t world,
                          void *d_scratch, int32_t *d_req_rows, int32_t *d_counts, int32_t *d_ci, int32_t *d_cj,
                          void *stream);
int qrec_shard_plan_epoch_scratch_bytes(int64_t n_items, int32_t world, int32_t n_batches, int64_t *bytes);
int qrec_shard_plan_epoch(const int32_t *d_i, const int32_t *d_j, const int64_t *d_bounds, int32_t n_batches, int64_t n,
                          int64_t n_items, int32_t world, void *d_scratch, int32_t *d_req_rows, const int64_t *d_req_off,
                          int32_t *d_counts, int32_t *d_ci, int32_t *d_cj, void *stream);
int qrec_gather_rows(const float *d_table, int32_t ld, const int32_t *d_rows, int64_t n, float *d_out, void *stream);
/* The rows of a training batch out of / into ROW-PARTITIONED tables (graph models; the rows tf.nn.embedding_lookup
 * reads, model/ranking/LightGCN.py:22-24).  Batch row k of 3B is table row u[k] (k < B), n_users + i[k - B] (k < 2B) or
 * n_users + j[k - 2B]; d_block holds the table's rows [lo, hi).
 * qrec_batch_rows_gather:       d_out[k] = the row if lo <= row < hi, else zeros ([3B][ld]): summed over the ranks (one all-reduce of
 *                               3B rows) these are the batch's rows of the whole table -- instead of an all-gather of the table;
 * qrec_batch_rows_scatter_add:  d_block[row(k) - lo] += d_src[k] for every k whose row lies in [lo, hi) (f32 atomics: a batch
 *                               repeats rows; lo = 0, hi = N scatters into a whole table).                                      */
/* ... and for an arbitrary list of table rows d_ids[n] (SimGCL's InfoNCE reads the batch's UNIQUE users / items, SimGCL.py:61-64) */
int qrec_rows_gather_owned(const float *d_block, int32_t ld, int64_t lo, int64_t hi, const int32_t *d_ids, int64_t n, float *d_out, void *stream);
int qrec_rows_scatter_add_owned(float *d_block, int32_t ld, int64_t lo, int64_t hi, const int32_t *d_ids, int64_t n, const float *d_src, void *stream);
int qrec_batch_rows_gather(const float *d_block, int32_t ld, int64_t lo, int64_t hi, const int32_t *d_u, const int32_t *d_i,
                           const int32_t *d_j, int32_t B, int64_t n_users, float *d_out, void *stream);
int qrec_batch_rows_scatter_add(float *d_block, int32_t ld, int64_t lo, int64_t hi, const int32_t *d_u, const int32_t *d_i,
                                const int32_t *d_j, int32_t B, int64_t n_users, const float *d_src, void *stream);
int qrec_scatter_add_row_deltas(float *d_table, int32_t ld, const int32_t *d_rows, int64_t n, const float *d_fresh,
                                const float *d_sent, void *stream);

/* ---- alternating least squares, fp64 (model/ranking/WRMF.py:17-67; als.hip) ------------------------------------------ *
 * Tables are fp64 [rows][ld], ld in {16, 32, 64, 128} (engine.padded_ld), 1 <= d <= ld, pad columns zero.
 * qrec_als_gram: d_G[ld][ld] = F^T F over the whole padded rows (the pad block comes out zero).  Fixed partition of the
 *   rows over the blocks, partials added in block order: bit-reproducible.  Workspace: qrec_als_gram_workspace_bytes.
 * qrec_als_solve_rows: for every row r of the CSR (d_indptr[n_rows + 1], d_indices into the rows of d_F, d_c per entry)
 *       A_r = G + sum c f f^T + lambda I   (leading d x d block),   b_r = sum (1 + c) f,   X[r] = A_r^-1 b_r   (Cholesky)
 *   and, when d_loss is not NULL, *d_loss = sum_r sum_k (1 - X_old[r] . f_k)^2 with the rows of X before this call
 *   (WRMF.py:37-38).  Rows with more than QREC_ALS_SPLIT_DEGREE entries are accumulated in QREC_ALS_SEGMENT-entry segments
 *   on blocks of their own and their partials added in segment order; every sum has a fixed order (bit-reproducible).
 *   X is written only when every row succeeded: a non-positive (or NaN) pivot returns QREC_ERR_NOT_SPD, an index outside
 *   [0, f_rows) or a decreasing indptr QREC_ERR_INVALID, and X and *d_loss are left as they were.  The call waits for
 *   its stream (it reads the status back).  Workspace: qrec_als_solve_workspace_bytes over the same indptr, on the host. */
#define QREC_ALS_MAX_D 128
#define QREC_ALS_SEGMENT 256
#define QREC_ALS_SPLIT_DEGREE 512
int qrec_als_gram_workspace_bytes(int64_t rows, int32_t ld, int64_t *bytes);
int qrec_als_gram(const double *d_F, int64_t rows, int32_t d, int32_t ld, double *d_G, void *d_ws, int64_t ws_bytes, void *stream);
int qrec_als_solve_workspace_bytes(const int64_t *h_indptr, int64_t n_rows, int32_t ld, int64_t *bytes);
int qrec_als_solve_rows(const double *d_F, int64_t f_rows, const double *d_G, double *d_X, int64_t n_rows, int32_t d, int32_t ld,
                        const int64_t *d_indptr, const int32_t *d_indices, const double *d_c, double lambda, double *d_loss,
                        void *d_ws, int64_t ws_bytes, void *stream);

/* ---- CoFactor, fp64 (model/ranking/CoFactor.py; cofactor.hip) ---------------------------------------------------------- *
 * Co-occurrence (CoFactor.py:36-56).  The binary rating matrix as two CSR views: d_i_indptr[n_items + 1] / d_i_users[i_nnz] (the
 * raters of every item) and d_u_indptr[n_users + 1] / d_u_items[u_nnz] (every user's items, ascending, no duplicates).
 * count(i, j) = the users who rated both; the pair (i, j), i != j, is kept when count > filter and both items have >= filter
 * raters (filter >= 0).  Integer arithmetic throughout: the result does not depend on any order.
 * qrec_cooc_count: *kept = the number of kept directed pairs (both (i, j) and (j, i) count); leaves the per-(item, tile)
 *   offsets in the workspace for qrec_cooc_fill.  Waits for its stream.  Workspace: qrec_cooc_workspace_bytes.
 * qrec_cooc_fill: after qrec_cooc_count of the same inputs and workspace, the kept pairs as a CSR: d_out_indptr[n_items + 1],
 *   d_out_cols / d_out_counts[capacity], columns ascending within a row.  More kept pairs than capacity: QREC_ERR_INVALID and
 *   nothing written.  Waits for its stream.
 * An index outside its table or an indptr that decreases or passes its nnz returns QREC_ERR_INVALID (the outputs are then undefined
 * but every access stayed in bounds).
 *
 * Item step (CoFactor.py:116-159).  Tables as for ALS: fp64 [rows][ld], ld in {16, 32, 64, 128}, 1 <= d <= ld, pad columns zero;
 * d_w, d_c fp64 [n_items].  d_XtX = X^T X (qrec_als_gram).  Ratings by item: d_r_indptr[n_items + 1], d_r_users, d_r_conf[r_nnz].
 * Contexts by item: d_s_indptr[n_items + 1], d_s_items, d_s_vals[s_nnz] (the SPPMI rows, in the order their sums are to be
 * taken).  For item i with contexts k, s = its value, from the rows as they are when the step runs:
 *     Y[i] = (XtX + sum_u conf x x^T + lambda I + sum_k g_k g_k^T)^-1 (sum_u (1 + conf) x + sum_k (s - w_i - c_k) g_k)
 *     G[i] = (sum_k y_k y_k^T + gamma I)^-1 sum_k (s - w_k - c_i) y_k
 *     w[i] = mean_k (s - Y_old[i] . g_k - c_k),   c[i] = mean_k (s - y_k . G_old[i] - w_k)
 * (Cholesky; w_i, c_i in the sums are the old values).  d_order[h_level_ptr[n_levels]] lists the items with contexts level by
 * level (h_level_ptr on the host): the items of one level must not be contexts of one another; the levels run in order, one
 * launch each, so a step sees the rows written by the earlier levels -- with level(i) = 1 + max level(earlier context) this is
 * the reference's sequential sweep.  d_solo[n_solo] lists the items without contexts, solved as plain ALS rows (only Y[i]
 * changes); items in neither list are left alone.  Every sum has a fixed order: bit-reproducible.  The sweep runs on copies
 * of Y, G, w, c in the workspace, copied back only when every system was positive definite: QREC_ERR_NOT_SPD (naming the
 * smallest failing item), an index outside its table or a bad indptr (QREC_ERR_INVALID) leave all four as they were.  Waits for
 * its stream.  Workspace: qrec_cofactor_item_workspace_bytes(n_items, number of scheduled items, ld). */
#define QREC_COOC_TILE 8192
int qrec_cooc_workspace_bytes(int64_t n_items, int64_t *bytes);
int qrec_cooc_count(const int64_t *d_i_indptr, const int32_t *d_i_users, int64_t n_items, int64_t i_nnz, const int64_t *d_u_indptr,
                    const int32_t *d_u_items, int64_t n_users, int64_t u_nnz, int32_t filter, int64_t *kept, void *d_ws,
                    int64_t ws_bytes, void *stream);
int qrec_cooc_fill(const int64_t *d_i_indptr, const int32_t *d_i_users, int64_t n_items, int64_t i_nnz, const int64_t *d_u_indptr,
                   const int32_t *d_u_items, int64_t n_users, int64_t u_nnz, int32_t filter, int64_t *d_out_indptr,
                   int32_t *d_out_cols, int32_t *d_out_counts, int64_t capacity, void *d_ws, int64_t ws_bytes, void *stream);
int qrec_cofactor_item_workspace_bytes(int64_t n_items, int64_t n_ctx_items, int32_t ld, int64_t *bytes);
int qrec_cofactor_item_rows(const double *d_X, int64_t n_users, const double *d_XtX, double *d_Y, double *d_G, double *d_w, double *d_c,
                            int64_t n_items, int32_t d, int32_t ld, const int64_t *d_r_indptr, const int32_t *d_r_users,
                            const double *d_r_conf, int64_t r_nnz, const int64_t *d_s_indptr, const int32_t *d_s_items,
                            const double *d_s_vals, int64_t s_nnz, const int32_t *d_order, const int32_t *h_level_ptr,
                            int32_t n_levels, const int32_t *d_solo, int64_t n_solo, double lambda, double gamma, void *d_ws,
                            int64_t ws_bytes, void *stream);

/* ---- exposure-weighted ALS, fp64 (model/ranking/ExpoMF.py, model/ranking/SERec.py; exposure.hip) --------------------- *
 * Tables as for ALS: fp64 [rows][ld], ld in {16, 32, 64, 128}, 1 <= d <= ld, pad columns zero; d > QREC_ALS_MAX_D returns
 * QREC_ERR_UNSUPPORTED.  The exposure posterior of (row r, column c), from the row's table X and the column's table F:
 *     pEX = sqrt(lam_y / 2 pi) exp(-lam_y (X[r] . F[c])^2 / 2),   A_rc = (pEX + 1e-8) / (pEX + 1e-8 + (1 - mu_rc) / mu_rc)
 * with the prior mu_rc given by qrec_expo_prior_t:
 *   QREC_EXPO_PRIOR_COL           mu_rc = v[c]                    (ExpoMF, user half)
 *   QREC_EXPO_PRIOR_ROW           mu_rc = v[r]                    (ExpoMF, item half)
 *   QREC_EXPO_PRIOR_SOCIAL_T_ROW  mu_rc = m(t[r], a_sum[c])       (SERec, user half)
 *   QREC_EXPO_PRIOR_SOCIAL_T_COL  mu_rc = m(t[c], a_sum[r])       (SERec, item half)
 *   m(t, A) = (a + A + (s - 1) t A - 1) / (a + b + (s - 1) t A + n_users - 2)   (SERec.py:92-95; T.dot(tile(A_sum)) = t_u A_i)
 * qrec_expo_solve_rows: for every row r of X (its observed columns: d_indptr[n_rows + 1] / d_indices, unique within a row)
 *       B_r = sum_{c < n_cols} A_rc F[c] F[c]^T + lambda I   with A_rc = 1 on the observed columns,
 *       b_r = sum_{c observed} F[c],   X[r] = B_r^-1 b_r   (Cholesky; A from X's rows before this call)
 *   on f64 MFMA, every sum in a fixed order (bit-reproducible).  X is written only when every row succeeded: a non-positive
 *   (or NaN) pivot returns QREC_ERR_NOT_SPD, an index outside [0, n_cols) or a decreasing indptr QREC_ERR_INVALID, and X
 *   is left as it was.  Waits for its stream.  Workspace: qrec_expo_solve_workspace_bytes.
 * qrec_expo_prior: the prior pass over rows = users (X, n_rows) and columns = items (F, n_cols), the columns' observed rows
 *   given by d_col_indptr / d_col_indices:  d_a_sum[c] = sum_r A_rc (A = 1 on observed pairs), summed over a fixed
 *   partition of the rows in a fixed order; when d_mu is not NULL also d_mu[c] = (a + A_c - 1) / (a + b + n_users - 2)
 *   (ExpoMF.py:73).  d_a_sum / d_mu may alias the prior's own vectors (they are written after every read).  Nothing is
 *   written on QREC_ERR_INVALID.  Waits for its stream.  Workspace: qrec_expo_prior_workspace_bytes. */
#define QREC_EXPO_PRIOR_COL 0
#define QREC_EXPO_PRIOR_ROW 1
#define QREC_EXPO_PRIOR_SOCIAL_T_ROW 2
#define QREC_EXPO_PRIOR_SOCIAL_T_COL 3
typedef struct {
    int32_t mode;
    int32_t reserved;
    const double *v;       /* modes COL / ROW */
    const double *t;       /* social modes: followee counts per user */
    const double *a_sum;   /* social modes: A_sum per item */
    double a, b, s, n_users, lam_y;
} qrec_expo_prior_t;
int qrec_expo_solve_workspace_bytes(int64_t n_rows, int32_t ld, int64_t *bytes);
int qrec_expo_solve_rows(const double *d_F, int64_t n_cols, double *d_X, int64_t n_rows, int32_t d, int32_t ld,
                         const int64_t *d_indptr, const int32_t *d_indices, const qrec_expo_prior_t *prior, double lambda,
                         void *d_ws, int64_t ws_bytes, void *stream);
int qrec_expo_prior_workspace_bytes(int64_t n_rows, int64_t n_cols, int64_t *bytes);
int qrec_expo_prior(const double *d_X, int64_t n_rows, const double *d_F, int64_t n_cols, int32_t d, int32_t ld,
                    const int64_t *d_col_indptr, const int32_t *d_col_indices, const qrec_expo_prior_t *prior, double *d_a_sum,
                    double *d_mu, void *d_ws, int64_t ws_bytes, void *stream);

/* ---- memory-based rating models, fp64 (model/rating/{UserKNN,ItemKNN,SlopeOne}.py, util/qmath.py:19-115; knn.hip) ----- *
 * No FMA contraction; every sum runs in the reference's order; no float atomics: a run is bit-identical to the next.
 * qrec_knn_sweep: for every query t < n_queries (its row: d_q_keys / d_q_vals[d_q_indptr[t] .. d_q_indptr[t + 1]), in the
 *   reference's dict order) and every candidate label c < n_cands, the similarity of the query's row (x1) and the candidate's
 *   row (x2) over their common keys, summed in x1's order:
 *     PCC        sum (a - m1)(b - m2) / (sqrt(sum (a - m1)^2) sqrt(sum (b - m2)^2)), m1 = d_q_means[t], m2 = d_c_means[c];
 *                a zero denominator gives 1 when a key overlapped, else 0
 *     COS        sum ab / (sqrt(sum a^2) sqrt(sum b^2)); a zero denominator gives 0
 *     EUCLIDEAN  1 / sum (a^2 - b^2); a zero total gives 0
 *     SLOPEONE   sum (a - b) / count (0 when count = 0), and d_count_out[t][c] = count
 *   into d_out[t * ld_out + c].  Every square is an input, per entry: d_q_sq / d_c_sq = pow((a - m1), 2) / pow((b - m2), 2)
 *   for PCC, pow(a, 2) / pow(b, 2) for COS and EUCLIDEAN, as the C library's pow gives them (the reference's ``x ** 2``);
 *   unused (NULL) for SLOPEONE.  The candidates' rows are given inverted: key -> (label, value) in d_c_labels / d_c_vals
 *   [d_c_indptr[key] .. d_c_indptr[key + 1]), labels ascending within a key.  One workgroup per (query, QREC_KNN_TILE labels).
 * qrec_knn_topk: query t's neighbour sequence is, when d_q_label[t] = j >= 0 (the query is the candidate
 *   with label j; labels 0 .. m - 1 are the queries that are candidates, in query order): the earlier queries s < t with the
 *   value d_S[s][j] (id d_test_code[s]), then the labels c > j with the value d_S[t][c] (id d_lab2id[c]); when j < 0: every
 *   label c with d_S[t][c].  Each query's first k entries of the stable sort by value, descending (-0.0 == 0.0), go to
 *   d_ids / d_vals[t * k ..] and their number to d_counts[t].  k > QREC_KNN_MAX_K returns QREC_ERR_UNSUPPORTED.
 *   Workspace (the transposed query x query block): qrec_knn_topk_workspace_bytes.
 * qrec_knn_predict: for every row r, the first d_nb_counts[q] neighbours n of query q = d_row_query[r] in order: mode 0
 *   (UserKNN) looks up key d_row_other[r] (item) in member row n, mode 1 (ItemKNN) key n in member row d_row_other[r] (user);
 *   the member rows (d_m_indptr / d_m_keys ascending / d_m_vals) are the users' ratings.  Found: sum += s (r - d_nb_means[n]),
 *   denom += s.  sum == 0: d_pred = d_row_base[r], status FALLBACK; denom == 0: status ZERO_DIVISION; else
 *   d_pred = d_row_base[r] + sum / denom, status COMPUTED.
 * qrec_slopeone_batch: the SLOPEONE sweep of queries [q0, q0 + nq) (test items; candidates: all items) into the workspace
 *   (qrec_slopeone_workspace_bytes(nq, n_items)), then every row r whose query lies in the batch: user u = d_row_user[r] >= 0
 *   walks its row in dict order (d_u_indptr / d_u_items / d_u_vals): sum += (r + dev) * freq, freqSum += freq;
 *   d_pred = sum / freqSum (COMPUTED), or d_row_base[r] when freqSum == 0 or u < 0 (FALLBACK).  d_u_*_sorted are the same
 *   rows with the items ascending (the sweep's inverted index). */
#define QREC_KNN_PCC 0
#define QREC_KNN_COS 1
#define QREC_KNN_EUCLIDEAN 2
#define QREC_KNN_SLOPEONE 3
#define QREC_KNN_TILE 2048
#define QREC_KNN_MAX_K 256
#define QREC_KNN_COMPUTED 0
#define QREC_KNN_FALLBACK 1
#define QREC_KNN_ZERO_DIVISION 2
int qrec_knn_sweep(int32_t measure, int64_t n_queries, const int64_t *d_q_indptr, const int32_t *d_q_keys, const double *d_q_vals,
                   const double *d_q_means, const double *d_q_sq, int64_t n_keys, const int64_t *d_c_indptr, const int32_t *d_c_labels,
                   const double *d_c_vals, const double *d_c_sq, int64_t n_cands, const double *d_c_means, double *d_out, int64_t ld_out, int32_t *d_count_out, int64_t ld_count,
                   void *stream);
int qrec_knn_topk_workspace_bytes(int64_t n_queries, int64_t m, int64_t *bytes);
int qrec_knn_topk(int64_t n_queries, const double *d_S, int64_t ld_S, int64_t m, const int32_t *d_q_label, const int32_t *d_test_code,
                  const int32_t *d_lab2id, int64_t n_cands, int32_t k, int32_t *d_ids, double *d_vals, int32_t *d_counts, void *d_ws,
                  int64_t ws_bytes, void *stream);
int qrec_knn_predict(int32_t mode, int64_t n_rows, const int32_t *d_row_query, const int32_t *d_row_other, const double *d_row_base,
                     const int32_t *d_nb_ids, const double *d_nb_vals, const int32_t *d_nb_counts, int64_t n_queries, int32_t k,
                     int64_t n_members, const int64_t *d_m_indptr, const int32_t *d_m_keys, const double *d_m_vals, int64_t n_nb,
                     const double *d_nb_means, double *d_pred, int32_t *d_status, void *stream);
int qrec_slopeone_workspace_bytes(int64_t batch, int64_t n_items, int64_t *bytes);
int qrec_slopeone_batch(int64_t q0, int64_t nq, const int64_t *d_q_indptr, const int32_t *d_q_keys, const double *d_q_vals,
                        int64_t n_users, const int64_t *d_u_indptr_sorted, const int32_t *d_u_items_sorted, const double *d_u_vals_sorted,
                        int64_t n_items, int64_t n_rows, const int32_t *d_row_query, const int32_t *d_row_user, const double *d_row_base,
                        const int64_t *d_u_indptr, const int32_t *d_u_items, const double *d_u_vals, double *d_pred, int32_t *d_status,
                        void *d_ws, int64_t ws_bytes, void *stream);


/* ---- social-trust rating models (model/rating/{SoRec,SoReg,SocialMF,RSTE,SREE}.py), fp64 tables, order-exact ----------
 * qrec_rste_sgd_ordered: RSTE.py:22-40 strictly in array order (one wavefront).  d_fe_indptr [n_users+1] / d_fe_ids / d_fe_w:
 *   every user's followees in dict order with their weights; d_fe_den [n_users]: their weight sum as the host's numpy gives
 *   it.  den != 0: pred = alpha*P[u].Q[i] + ((1-alpha)*sum_f w_f P[f].Q[i])/den, else P[u].Q[i]; *d_loss = sum(error^2).
 * qrec_social_user_pass: the per-user social pass, mode QREC_SOCIAL_SOCIALMF (SocialMF.py:25-41, coef = regS),
 *   QREC_SOCIAL_SOREG (SoReg.py:58-74, coef = alpha) or QREC_SOCIAL_SREE (SREE.py:50-63, coef = alpha).  Step k is user
 *   d_step_user[k]; its followees are d_fe_ids[d_fe_indptr[k] ..] with weights d_fe_w (SoReg: Sim per edge), its followers
 *   (SoReg only) d_fr_*.  Loss terms go to d_slots: one per step for SocialMF, one per followee edge for SoReg and SREE.
 * qrec_sorec_relation_pass: SoRec.py:41-58 over relations k = (d_rel_u, d_rel_v, d_rel_t) with the weight d_rel_w;
 *   d_slots[k] = regS*euv^2.
 * Both social passes run the level schedule d_order / d_level_ptr [n_levels+1] (steps of level L: d_order[d_level_ptr[L] ..
 *   d_level_ptr[L+1]), no two of them conflicting on a row) in one workgroup of n_waves (1..QREC_SOCIAL_MAX_WAVES)
 *   wavefronts; any valid schedule gives the bits of the sequential walk.
 * qrec_loss_fold: *d_running = ((*d_running + d_slots[0]) + d_slots[1]) + ... in slot order.                          */
#define QREC_SOCIAL_SOCIALMF 0
#define QREC_SOCIAL_SOREG 1
#define QREC_SOCIAL_SREE 2
#define QREC_SOCIAL_MAX_WAVES 16
int qrec_rste_sgd_ordered(double *d_P, double *d_Q, int32_t d, int32_t ld, const int64_t *d_fe_indptr, const int32_t *d_fe_ids,
                          const double *d_fe_w, const double *d_fe_den, const int32_t *d_u, const int32_t *d_i,
                          const double *d_rating, int64_t n, double lr, double alpha, double regU, double regI, double *d_loss,
                          void *stream);
int qrec_social_user_pass(int mode, double *d_P, int32_t d, int32_t ld, const int32_t *d_step_user, int64_t n_steps,
                          const int64_t *d_fe_indptr, const int32_t *d_fe_ids, const double *d_fe_w, const int64_t *d_fr_indptr,
                          const int32_t *d_fr_ids, const double *d_fr_w, const int32_t *d_order, const int32_t *d_level_ptr,
                          int32_t n_levels, int32_t n_waves, double lr, double coef, double *d_slots, void *stream);
int qrec_sorec_relation_pass(double *d_P, double *d_Z, int32_t d, int32_t ld, const int32_t *d_rel_u, const int32_t *d_rel_v,
                             const double *d_rel_t, const double *d_rel_w, int64_t n_rel, const int32_t *d_order,
                             const int32_t *d_level_ptr, int32_t n_levels, int32_t n_waves, double lr, double regS, double regZ,
                             double *d_slots, void *stream);
int qrec_loss_fold(double *d_running, const double *d_slots, int64_t n, void *stream);

/* ---- LOCABAL and SocialFD (model/rating/{LOCABAL,SocialFD}.py): passes that carry a dense d x d matrix H, fp64, order-exact
 * d_H is row-major [d][d] doubles in global memory; a launch keeps it in LDS ([d][d | 1]) and writes it back at the end.
 * Supported width: d <= QREC_SOCIAL_H_MAX_D (H then takes 129 KiB of the CU's 160 KiB); a wider call returns
 * QREC_ERR_UNSUPPORTED from all four entries and touches nothing.  Every step conflicts with every other through H, so ONE
 * workgroup of n_waves wavefronts (1..QREC_SOCIAL_MAX_WAVES, 0 = chosen from d; never fewer than ceil(d / 64), one thread
 * per column) walks a pass step by step and works side by side inside a step.  Sums over d terms are formed as partial sums over 16 consecutive terms, each added one term after the
 * other, then added in chunk order; that association depends on d alone, so every n_waves gives the same bits, as do two
 * launches.  No float atomics.  The metric products H.H^T + (H.H^T)^T (SocialFD.py:44) and H.H^T + H^T.H (:82) are never
 * formed: (H.H^T).v is computed as H.(H^T.v).
 * qrec_locabal_sgd_ordered: LOCABAL.py:50-67 in array order (one wavefront).  d_w_user [n_users]: W[user], or 0 for a user
 *   in no relation (a real weight is > 0).  p, q are copies; a user with a weight gets the weighted update and then the
 *   plain one (the reference's `else` is commented out).  *d_loss = sum of w*err^2 or err^2, added in row order.
 * qrec_locabal_social_pass: LOCABAL.py:68-80 over the edges (d_edge_u, d_edge_k, d_edge_sim) in order: e = sim - (p^T H).q;
 *   H += ((lr*alpha)*e)*(p_i*q_j); H -= (lr*regS)*H; P[u] += ((lr*alpha)*e)*(H q); P[k] += ((lr*alpha)*e)*(p^T H), both on
 *   the new H and the old p (k == u: onto the row just written).  d_slots[edge] = alpha*e^2.
 * qrec_socialfd_sgd_ordered: SocialFD.py:28-72 in array order, x = P[u] and y = Q[i] being VIEWS as in the reference.  The
 *   bands are r > 0.7, r <= 0.5 (two branches: distance < 1, >= 1) and the rest; *d_loss adds err^2 and then the band's
 *   term per rating.  Bu, Bi are updated with regU, regI as the reference does.
 * qrec_socialfd_social_pass: SocialFD.py:74-86; step k is user d_step_user[k] (data.user order) with followees
 *   d_fe_ids[d_fe_indptr[k] ..] in dict order: per followee the metric term to d_slots[edge], P[u] -= ((lr*eta)*beta)*delta
 *   and H -= ((lr*eta)*beta)*(H*(w.w)).                                                                                    */
#define QREC_SOCIAL_H_MAX_D 128
int qrec_locabal_sgd_ordered(double *d_P, double *d_Q, int32_t d, int32_t ld, const double *d_w_user, const int32_t *d_u,
                             const int32_t *d_i, const double *d_rating, int64_t n, double lr, double regU, double regI,
                             double *d_loss, void *stream);
int qrec_locabal_social_pass(double *d_P, double *d_H, int32_t d, int32_t ld, const int32_t *d_edge_u, const int32_t *d_edge_k,
                             const double *d_edge_sim, int64_t n_edges, int32_t n_waves, double lr, double alpha, double regS,
                             double *d_slots, void *stream);
int qrec_socialfd_sgd_ordered(double *d_P, double *d_Q, double *d_Bu, double *d_Bi, double *d_H, int32_t d, int32_t ld,
                              const int32_t *d_u, const int32_t *d_i, const double *d_rating, int64_t n, int32_t n_waves, double lr,
                              double regU, double regI, double eta, double alpha, double global_mean, double *d_loss, void *stream);
int qrec_socialfd_social_pass(double *d_P, double *d_H, int32_t d, int32_t ld, const int32_t *d_step_user, int64_t n_steps,
                              const int64_t *d_fe_indptr, const int32_t *d_fe_ids, int32_t n_waves, double lr, double eta, double beta,
                              double *d_slots, void *stream);

/* ---- evaluation of the rating models (csrc/rating_eval.hip): base/recommender.py:88-110, every predictForRating --------------
 * fp64 tables only (dtype must be QREC_F64: anything else returns QREC_ERR_INVALID and launches nothing), no float atomics,
 * the same bits from launch to launch.  Test pairs are (d_uid[t], d_iid[t]); -1 = a name the training set does not know
 * (any id outside its table is treated like -1 and never dereferenced).  One wavefront evaluates one pair, lane = column,
 * in a grid-stride loop of at most QREC_RATING_MAX_BLOCKS workgroups of QREC_RATING_BLOCK_WAVES wavefronts.  A dot product
 * is one fixed tree; the scalar sums after it are added left to right as the class adds them:
 *   QREC_RATING_DOT     P[u].Q[i]; only the user known: d_user_mean[u]; only the item: d_item_mean[i]; neither: global_mean
 *   QREC_RATING_BIASED  ((P[u].Q[i] + mean) + Bi[i]) + Bu[u];                     either side unknown: global_mean (all below)
 *   QREC_RATING_SVDPP   imp[u].Q[i] + the BIASED value; d_aux = imp [n_users][ld] from qrec_rating_implicit
 *   QREC_RATING_EUCLID  ((mean + Bi[i]) + Bu[u]) - diff.diff, diff = P[u] - Q[i]
 *   QREC_RATING_METRIC  ((Bi[i] + Bu[u]) + mean) - ((diff.H).H^T).diff; d_aux = H [d][d], staged in LDS as [d][d | 1];
 *                       d > QREC_SOCIAL_H_MAX_D returns QREC_ERR_UNSUPPORTED and launches nothing
 *   QREC_RATING_RSTE    alpha*P[u].Q[i] + ((1-alpha)*sum_f w_f (P[f].Q[i]))/den[u] where den[u] != 0, else P[u].Q[i], over the
 *                       followee CSR of qrec_rste_sgd_ordered
 * d_pred[t] receives the UNROUNDED prediction.  Arrays a form does not read may be null.
 * qrec_rating_implicit: imp[u] = (...((Y[j0] + Y[j1]) + Y[j2])...) / count over d_rated_items[d_rated_indptr[u] ..] in that
 *   order, for the n users of d_users (each once); rows of other users are left as they are.
 * qrec_rating_boundary: in place, x > hi -> hi, x < lo -> lo, else Python's round(x, 3) (half to even on the exact decimal
 *   value of the double).
 * qrec_rating_errors: d_abs[t] = |r - p|, d_sq[t] = (r - p)*(r - p); qrec_loss_fold adds either array in pair order.      */
#define QREC_RATING_DOT 0
#define QREC_RATING_BIASED 1
#define QREC_RATING_SVDPP 2
#define QREC_RATING_EUCLID 3
#define QREC_RATING_METRIC 4
#define QREC_RATING_RSTE 5
#define QREC_RATING_BLOCK_WAVES 8
#define QREC_RATING_MAX_BLOCKS 256
int qrec_rating_implicit(const double *d_Y, int32_t dtype, int32_t n_items, int32_t d, int32_t ld, const int64_t *d_rated_indptr,
                         const int32_t *d_rated_items, const int32_t *d_users, int64_t n, int32_t n_users, double *d_imp,
                         void *stream);
int qrec_rating_predict(int32_t form, int32_t dtype, const double *d_P, const double *d_Q, int32_t n_users, int32_t n_items, int32_t d,
                        int32_t ld, const double *d_Bu, const double *d_Bi, const double *d_aux, const int64_t *d_fe_indptr,
                        const int32_t *d_fe_ids, const double *d_fe_w, const double *d_fe_den, const double *d_user_mean,
                        const double *d_item_mean, double global_mean, double alpha, const int32_t *d_uid, const int32_t *d_iid,
                        int64_t n, double *d_pred, void *stream);
int qrec_rating_boundary(double *d_x, int64_t n, double lo, double hi, void *stream);
int qrec_rating_errors(const double *d_rating, const double *d_pred, int64_t n, double *d_abs, double *d_sq, void *stream);

/* ---- ranking of the rating models (csrc/rank_forms.hip): predictForRanking of SVD, SVDPlusPlus, EE, SREE, RSTE, SocialFD -------
 * qrec_score_topk's BLOCK route with its scoring step replaced by one of the QREC_RATING_* forms above, fp64, no float atomics,
 * the same bits from launch to launch; mask (rated items -> 0) and the reference's heap top-N run unchanged, outputs are
 * [n_batch_users][N] with ids -1-padded when n_items < N.  Score of (user u, item i), mu = the global mean:
 *   QREC_RATING_DOT     Q[i].P[u]
 *   QREC_RATING_BIASED  ((Q[i].P[u] + mu) + Bi[i]) + Bu[u]                                                    (SVD.py:88)
 *   QREC_RATING_SVDPP   the BIASED value on the row P[u] + (sum_j Y[j]) / w over d_y_items[d_y_indptr[u] ..] in that order
 *                       (userRated order; w = the row's length, w = 0: P[u] alone)                     (SVDPlusPlus.py:90-103)
 *   QREC_RATING_EUCLID  ((sign * |Q[i] - P[u]|^2 + Bi[i]) + Bu[u]) + mu, sign = +1 for EE.py:93 / SREE.py:77, which rank by the
 *                       distance itself; |x - y|^2 is formed as (|y|^2 - 2 y.x) + |x|^2
 *   QREC_RATING_METRIC  the EUCLID value on the rows P[u].H and Q[i].H, sign = -1 for SocialFD.py:104-112 (d_H [d][d], staged in
 *                       LDS; d > QREC_SOCIAL_H_MAX_D returns QREC_ERR_UNSUPPORTED and writes nothing)
 *   QREC_RATING_RSTE    Q[i].e, e = alpha P[u] + ((1 - alpha) sum_f w_f P[f]) / den[u] over the followee CSR of
 *                       qrec_rste_sgd_ordered in its order, e = P[u] where den[u] == 0                        (RSTE.py:66-81)
 * Arrays a form does not read may be null; an item or followee id outside its table is skipped, never dereferenced.
 * qrec_rank_form_prepare: the item side, once per table upload, into a caller-owned buffer of qrec_rank_form_prepare_bytes
 *   (EUCLID: |Q[i]|^2; METRIC: Q.H [n_items][ld] and its squared row norms; the other forms need 0 bytes and the call does nothing).
 * qrec_score_topk_form: d_prep / prep_bytes = that buffer; d_scratch / scratch_bytes = qrec_score_topk_form_scratch_bytes.  Either
 *   buffer too small, a null pointer, ld not a multiple of 16, N outside 1..100 or half a rated CSR return QREC_ERR_INVALID before
 *   anything is written.  d_rated_indptr / d_rated_items (both or neither): the items to set to 0, any order inside a row. */
int qrec_rank_form_prepare_bytes(int32_t form, int32_t n_items, int32_t ld, int64_t *bytes);
int qrec_rank_form_prepare(int32_t form, const double *d_Q, const double *d_H, int32_t d, int32_t ld, int32_t n_items, void *d_prep,
                           int64_t prep_bytes, void *stream);
int qrec_score_topk_form_scratch_bytes(int32_t form, int32_t n_items, int32_t n_batch_users, int32_t ld, int32_t N, int64_t *bytes);
int qrec_score_topk_form(int32_t form, double sign, const double *d_P, const double *d_Q, int32_t d, int32_t ld, int32_t n_users,
                         int32_t n_items, const double *d_Bu, const double *d_Bi, double mu, const double *d_Y,
                         const int64_t *d_y_indptr, const int32_t *d_y_items, const double *d_H, const int64_t *d_fe_indptr,
                         const int32_t *d_fe_ids, const double *d_fe_w, const double *d_fe_den, double alpha, const void *d_prep,
                         int64_t prep_bytes, const int32_t *d_user_ids, int32_t n_batch_users, const int64_t *d_rated_indptr,
                         const int32_t *d_rated_items, int32_t N, void *d_scratch, int64_t scratch_bytes, int32_t *d_ids_out,
                         double *d_scores_out, void *stream);

/* ---- CDAE: model/ranking/CDAE.py (csrc/autoencoder.hip) -----------------------------------------------------------------
 * The denoising auto-encoder over a whole user row, evaluated only where the reference's dense batch x n_items arithmetic is
 * non-zero.  fp32; tables [rows][ld] with ld a multiple of 32 and columns [nh, ld) zero; the decoder weight is ITEM-MAJOR
 * ([n_items][ld], the transpose of the reference's variable).  Supported width: ld <= QREC_CDAE_MAX_LD, i.e. nh <= 256 --
 * a wider call returns QREC_ERR_UNSUPPORTED.  No float atomics: every sum has one order (list order inside a batch row, then
 * batch-row order), two launches give the same bits.  One batch of B rows (users d_users[b]) is described by
 *   the INPUT list: CSR over batch rows (d_in_ptr int32 [B+1], d_in_item, d_in_val) of the kept inputs (mask = 1 and rated),
 *     item ids ascending inside a row, and its item-major view (d_in_cptr [n_items+1], d_in_crow, d_in_cval), rows ascending;
 *   the LIVE list: CSR (d_lv_ptr, d_lv_item, d_lv_label 1 = positive / 0 = sampled negative) of the loss positions with
 *     mask = 1, ascending, and its item-major view (d_lv_cptr, d_lv_crow, d_lv_cslot = index of the entry in the CSR).
 *   Ids outside their table are skipped, never dereferenced.
 * qrec_cdae_encode:  h_b = sigmoid(sum x_bi Wenc[i] + benc + V[u_b]) summed in list order; h's padding columns are zero.
 * qrec_cdae_decode:  per live slot s = h_b . Wdec[i] + bdec[i], y = sigmoid(s), y^ = max(1e-6, y); the term is -log y^
 *   (positive) or -log(1 - y^) (negative), d_g[slot] = d term / d s / (B n_items) with the maximum's gradient passed only
 *   where y >= 1e-6; the workspace receives dh_b = sum g Wdec[i] as QREC_CDAE_SPLIT partial rows per batch row (each the
 *   in-order sum of a contiguous share of the row's slots) and the partial loss sums.
 * qrec_cdae_hidden_bwd:  dz_b = dh_b h_b (1 - h_b) (partials added in order), d_gbenc = sum_b dz_b, and
 *   d_gV[u_b] += dz_b + reg V[u_b] PER OCCURRENCE of a user (d_gV [n_users][ld] is zeroed first).
 * qrec_cdae_weight_grads: over the item-major views  gWdec[i] = sum g_bi h_b, gbdec[i] = sum g_bi, gWenc[i] = sum x_bi dz_b;
 *   rows of items absent from a view are written as exact zeros.  (reg * theta of Wenc, Wdec, benc, bdec: qrec_adam_step's grad_l2.)
 * qrec_cdae_loss: after decode and hidden_bwd of the same batch,  *d_loss = sum of the terms / (B n_items)
 *   + reg/2 (sum theta^2 over the n_theta contiguous floats of the four weight variables + sum_b |V[u_b]|^2).
 * Workspace: qrec_cdae_workspace_bytes(B, ld), shared by the three calls of a step. */
#define QREC_CDAE_MAX_LD 256
#define QREC_CDAE_SPLIT 8
#define QREC_CDAE_REG_BLOCKS 256
int qrec_cdae_workspace_bytes(int32_t B, int32_t ld, int64_t *bytes);
int qrec_cdae_encode(const float *d_Wenc, const float *d_benc, const float *d_V, int32_t n_items, int32_t n_users, int32_t nh,
                     int32_t ld, const int32_t *d_users, int32_t B, const int32_t *d_in_ptr, const int32_t *d_in_item,
                     const float *d_in_val, float *d_h, void *stream);
int qrec_cdae_decode(const float *d_Wdec, const float *d_bdec, int32_t n_items, int32_t nh, int32_t ld, const float *d_h, int32_t B,
                     const int32_t *d_lv_ptr, const int32_t *d_lv_item, const int32_t *d_lv_label, float *d_g, void *d_ws,
                     void *stream);
int qrec_cdae_hidden_bwd(const float *d_h, const float *d_V, int32_t n_users, int32_t nh, int32_t ld, const int32_t *d_users, int32_t B,
                         float reg, void *d_ws, float *d_dz, float *d_gbenc, float *d_gV, void *stream);
int qrec_cdae_weight_grads(const float *d_h, const float *d_dz, const float *d_g, int32_t n_items, int32_t nh, int32_t ld, int32_t B,
                           int64_t n_live, const int32_t *d_lv_cptr, const int32_t *d_lv_crow, const int32_t *d_lv_cslot,
                           const int32_t *d_in_cptr, const int32_t *d_in_crow, const float *d_in_cval, float *d_gWdec, float *d_gbdec,
                           float *d_gWenc, void *stream);
int qrec_cdae_loss(const float *d_theta, int64_t n_theta, float reg, int32_t B, int32_t n_items, int32_t ld, void *d_ws, double *d_loss,
                   void *stream);
/* qrec_cdae_draw_batch (throughput mode): one batch drawn and its lists built on the device, in the format above, so the
 * training calls do not know who fed them.  Same distribution as the reference's loop, not its streams: user of row b,
 * per_rated * |rated(user)| negatives by rejection against the user's rated row (ascending CSR over all users), and the keep
 * decision (probability keep_prob) of position (step, row, item) are Philox4x32-10 of (seed, step, position) -- the keep
 * decision is evaluated only at rated or sampled positions.  Negatives are a set per row (a bitmap over the items), lists come
 * out ascending.  cap_in / cap_live: capacities of the entry arrays; B * max row count and B * (1 + per_rated) * max row count
 * always suffice, pointers are clamped to them and no entry is written past them.  d_cand_count (may be null) receives per row
 * the number of positions whose keep decision was evaluated.  Integer atomics only; the result is a function of the arguments.
 * Workspace: qrec_cdae_draw_workspace_bytes(B, n_items). */
int qrec_cdae_draw_workspace_bytes(int32_t B, int32_t n_items, int64_t *bytes);
int qrec_cdae_draw_batch(const int64_t *d_rated_indptr, const int32_t *d_rated_items, const float *d_rated_vals, int32_t n_users,
                         int32_t n_items, int32_t B, int32_t per_rated, float keep_prob, uint64_t seed, uint64_t step, int64_t cap_in,
                         int64_t cap_live, void *d_ws, int32_t *d_users, int32_t *d_in_ptr, int32_t *d_in_item, float *d_in_val,
                         int32_t *d_in_cptr, int32_t *d_in_crow, float *d_in_cval, int32_t *d_lv_ptr, int32_t *d_lv_item,
                         int32_t *d_lv_label, int32_t *d_lv_cptr, int32_t *d_lv_crow, int32_t *d_lv_cslot, int32_t *d_cand_count,
                         void *stream);
/* qrec_mt_cdae_sample_batch (host): CDAE.py:21-43 on the CPython MT19937 stream -- per batch row user = choice(userList), then
 * per_rated * |rated(user)| draws of choice(itemList), each redrawn while the user rated it (rated CSR over all users).  Draws
 * per row in draw order, duplicates kept; the generator is left where the reference's loop leaves it. */
int qrec_mt_cdae_sample_batch(uint32_t *state625, const int64_t *rated_indptr, const int32_t *rated_items, int32_t n_users,
                              int32_t n_items, int32_t batch, int32_t per_rated, int32_t *users_out, int64_t *neg_indptr,
                              int32_t *neg_items, int64_t capacity);
/* qrec_score_topk's BLOCK route with S = sigmoid(S + d_item_bias[item]) between scoring and masking (CDAE.py:100-105 scores
 * sigmoid(h W + b), then base/recommender.py sets rated items to 0 -- on logits a rated item would outrank every item with a
 * negative logit).  fp32; d_U = the hidden rows [.][ld], d_V = the item-major decoder weight.  Scratch: its own size query. */
int qrec_score_topk_sigmoid_bias_scratch_bytes(int32_t n_items, int32_t n_batch_users, int64_t *bytes);
int qrec_score_topk_sigmoid_bias(const float *d_U, const float *d_V, const float *d_item_bias, int32_t d, int32_t ld, int32_t n_items,
                                 const int32_t *d_user_ids, int32_t n_batch_users, const int64_t *d_rated_indptr,
                                 const int32_t *d_rated_items, int32_t N, void *d_scratch, int32_t *d_ids_out, float *d_scores_out,
                                 void *stream);

/* ---- IRGAN: model/ranking/IRGAN.py (csrc/irgan.hip) ------------------------------------------------------------------------
 * A categorical distribution over the whole item table per user (tempered softmax, its CDF, many draws from it), the reward of
 * the drawn items, the policy-gradient step whose gradient is dense over the item table with TF's dense Adam, and the
 * discriminator's per-slot gradient rows.  Both towers score P[u] . Q[i] + b[i].
 * fp32 tables [rows][ld], ld one of 32 / 64 / 128 / 256, padding columns zero and kept zero.  An ITEM table carries its bias in
 * column d of the row ([Q | b]: d + 1 <= ld) and a user's row is read as [P[u] | 1], so one dot product is the logit and the
 * bias trains as one more column; a user table keeps columns >= d zero.  ld > QREC_IRGAN_MAX_LD or d + 1 > ld returns
 * QREC_ERR_UNSUPPORTED.  Ids outside a table are skipped, never dereferenced.  No float atomics: every sum has one order and two
 * launches give the same bits.  Plain launches on the caller's stream, no host read-back.
 *
 * qrec_irgan_row_weights: for the B users d_users[b] (positives: ascending CSR d_pos_indptr int64 [n_users + 1] / d_pos_items over
 *   ALL users), z_bj = ([P[u_b] | 1] . Qb[j]) / temperature into d_z [B][n_items], then with m = max_j z_bj
 *     QREC_IRGAN_NEGATIVES (get_data):  w = exp(z - m), 0 at the positives; d_p (may be null) receives exp(z - m) at every item;
 *     QREC_IRGAN_MIXTURE (generator):   p = exp(z - m) / sum_j exp(z_j - m) into d_p,  w = pn = (1 - sample_lambda) p, plus
 *                                       sample_lambda / |pos| at the positives.
 *   d_w [B][n_items] receives w and d_csum [B][ceil(n_items / QREC_IRGAN_CHUNK)] the INCLUSIVE prefix sums of w at the chunk
 *   ends, accumulated in fp64 in index order (inside a chunk, then chunk after chunk); the last one is the row total.
 *   The reference does not subtract m; the results differ only where its exp overflows float32 (z / T > 88).
 *   Workspace: qrec_irgan_row_workspace_bytes(B, n_items).  B <= 65535.
 * qrec_irgan_draw: row b takes the draws [d_draw_ptr[b], d_draw_ptr[b + 1]) (int64 [B + 1], n_draws in all).  Draw s of row b with
 *   uniform x in [0, 1) is the first item whose CDF value exceeds x (numpy's searchsorted(cdf, x, 'right') in np.random.choice):
 *   a binary search over the chunk sums for x * total, then the walk inside the chunk in the order its sum was formed, so a draw
 *   never lands on an item of zero weight.  x = d_uniforms[s], or, when d_uniforms is null, the 53-bit uniform of
 *   Philox4x32-10 keyed by (seed, step, row, index inside the row).  A row whose total is 0 draws -1.
 * qrec_irgan_uniforms: the uniforms qrec_irgan_draw uses when d_uniforms is null, d_out [n_draws].
 * qrec_irgan_reward: per sample  2 (sigmoid(x) - 1/2) d_p[b][i] / d_w[b][i]  with x = [P[u_b] | 1] . Qb[i] (P, Qb: the discriminator's),
 *   in float32 in that order, as the reference's graph forms it (its recorded losses carry the cancellation near x = 0).
 * qrec_irgan_gen_step (one user): with c_j = sum of the rewards of the samples equal to j in SAMPLE order (stable radix sort of
 *   (item, index) + walk), n_j their number, R = sum_k reward_k and K samples,  g_j = -(c_j - R p_j) / K  for every item,
 *     G[j] = g_j [P[u] | 1] + reg n_j Qb[j]     applied to Qb[j] by Adam in the same pass (the arithmetic of qrec_adam_step, alpha
 *     from the host) when apply != 0 -- no [n_items][ld] gradient exists unless d_gQ (may be null) asks for it; d_g (may be null)
 *     receives g;  d_gP[user] = sum_j g_j Qb[j][:d] (rows as read BEFORE their update; 64 items per workgroup in item order, then
 *     workgroup order) + reg P[user], the other rows of d_gP [n_users][ld] are not touched (keep them zero and hand the buffer to
 *     qrec_adam_step);  *d_loss (may be null) = -(1/K) sum_k log p[i_k] reward_k + reg (|P[u]|^2 + sum_k |Qb[i_k]|^2) / 2.
 *   Workspace: qrec_irgan_gen_workspace_bytes(n_items, ld, K).
 * qrec_irgan_dis_slots: per slot s (user d_u[s], item d_i[s], label d_label[s]) x = [P[u] | 1] . Qb[i], dz = sigmoid(x) - label,
 *     d_slotP[s] = dz Q[i] + B reg P[u],  d_slotQ[s] = dz [P[u] | 1] + B reg Qb[i]   (the reference minimises a [B] vector: the
 *     regulariser enters once per slot, B times over), d_keyP / d_keyQ = the destination rows (-1: a bad id) for
 *     qrec_scatter_add_rows_ordered, d_dz (may be null), d_terms [B] scratch, and
 *     *d_loss = sum_s (max(x, 0) - x label + log1p(exp(-|x|))) + B reg sum_s (|P[u]|^2 + |Qb[i]|^2) / 2.
 * qrec_irgan_assemble_rows: get_data's rows for a block of users on the device: row b owns [d_row_ptr[b], d_row_ptr[b + 1]) --
 *   its positives in CSR order with label 1, then its draws with label 0. */
#define QREC_IRGAN_MAX_LD 256
#define QREC_IRGAN_CHUNK 64
#define QREC_IRGAN_NEGATIVES 0
#define QREC_IRGAN_MIXTURE 1
int qrec_irgan_row_workspace_bytes(int32_t B, int32_t n_items, int64_t *bytes);
int qrec_irgan_row_weights(const float *d_P, const float *d_Q, int32_t n_users, int32_t n_items, int32_t d, int32_t ld,
                           const int32_t *d_users, int32_t B, const int64_t *d_pos_indptr, const int32_t *d_pos_items, int32_t mode,
                           float temperature, float sample_lambda, float *d_z, float *d_w, float *d_p, double *d_csum, void *d_ws,
                           void *stream);
int qrec_irgan_draw(const float *d_w, const double *d_csum, int32_t n_items, int32_t B, const int64_t *d_draw_ptr, int64_t n_draws,
                    const double *d_uniforms, uint64_t seed, uint64_t step, int32_t *d_samples, void *stream);
int qrec_irgan_uniforms(int32_t B, const int64_t *d_draw_ptr, int64_t n_draws, uint64_t seed, uint64_t step, double *d_out, void *stream);
int qrec_irgan_reward(const float *d_P, const float *d_Q, int32_t n_users, int32_t n_items, int32_t d, int32_t ld, const int32_t *d_users,
                      int32_t B, const int64_t *d_draw_ptr, int64_t n_draws, const int32_t *d_samples, const float *d_p, const float *d_w,
                      float *d_reward, void *stream);
int qrec_irgan_gen_workspace_bytes(int32_t n_items, int32_t ld, int64_t K, int64_t *bytes);
int qrec_irgan_gen_step(const float *d_P, float *d_Q, float *d_mQ, float *d_vQ, int32_t n_users, int32_t n_items, int32_t d, int32_t ld,
                        int32_t user, const int32_t *d_samples, const float *d_reward, int64_t K, const float *d_p, float reg, int32_t apply,
                        float alpha, float beta1, float beta2, float eps, float *d_gP, float *d_g, float *d_gQ, double *d_loss, void *d_ws,
                        int64_t ws_bytes, void *stream);
int qrec_irgan_dis_slots(const float *d_P, const float *d_Q, int32_t n_users, int32_t n_items, int32_t d, int32_t ld, const int32_t *d_u,
                         const int32_t *d_i, const float *d_label, int32_t B, float reg, float *d_slotP, float *d_slotQ, int32_t *d_keyP,
                         int32_t *d_keyQ, float *d_dz, double *d_terms, double *d_loss, void *stream);
int qrec_irgan_assemble_rows(const int32_t *d_users, int32_t n_users, int32_t B, const int64_t *d_pos_indptr, const int32_t *d_pos_items,
                             const int64_t *d_draw_ptr, const int32_t *d_samples, const int64_t *d_row_ptr, int64_t n_rows, int32_t *d_out_u,
                             int32_t *d_out_i, float *d_out_label, void *stream);

/* ---- CFGAN: model/ranking/CFGAN.py (csrc/cfgan.hip) -------------------------------------------------------------------------
 * Generator r^ = sigmoid(C G_W1 + G_b1) with G_W1 [n_items][ld] (ld a multiple of 32, >= n_items, padding columns zero and kept
 * zero) and G_b1 [ld]; discriminator D(x) = sigmoid(x . D_W1 + D_b1) over x = [r^ * mask | C] (fake) and [C | C] (real), its
 * 2 n_items + 1 values in ONE array d_thetaD (D_W1 flat, then D_b1).  The batch is in CDAE's list format with everything kept:
 * "in" = the rated entries of the batch rows (C[n,i] = in_val), "live" = the mask positions, and the per-slot array in the place
 * of lv_label is a FLAG: 1 where the position is in N_zr as well.  n_in / n_live are the entry counts (list pointers are clamped
 * to them, ids outside a table are skipped, never dereferenced).  fp32, fp64 loss sums, no float atomics: every sum has one order
 * (list order inside a batch row, ascending batch row inside an item) and two launches give the same bits.
 * n_items > QREC_CFGAN_MAX_ITEMS returns QREC_ERR_UNSUPPORTED (three n_items^2 fp32 tables must fit the device).
 *
 * qrec_cfgan_forward: at the live slots z = sum_i C[n,i] W[i][j] + b[j] (ascending i), r^ = sigmoid(z); per batch row the two
 *   logits, a_r = -(1/B) D_r (1 - D_r) / (D_r + 1e-4), a_f = (1/B) D_f (1 - D_f) / (1 - D_f + 1e-4) (1 - sigmoid(x) evaluated as
 *   sigmoid(-x)), delta = (-a_f D_W1[j] + alpha flag r^) r^ (1 - r^) per slot, and
 *     d_losses[0] = D_loss = -mean(log(D_r + 1e-4) + log(1 - D_f + 1e-4)),
 *     d_losses[1] = G_loss = mean log(1 - D_f + 1e-4) + alpha / 2 sum over flagged slots of r^2      -- all left in the workspace.
 * qrec_cfgan_dis_step (after forward on the same lists): the gradient of D_loss over the item-major views, real and fake pass
 *   summed apart and then added, and TF's Adam (alpha from the host) on the 2 n_items + 1 values in the same launch;
 *   d_grad_out (may be null) [2 n_items + 1] receives the gradient.
 * qrec_cfgan_gen_sweep (after forward): ONE pass over W, m, v -- each read once and written once in 16-byte accesses.  Per tile
 *   (row i, QREC_CFGAN_CHUNK columns) the gradient gW[i][j] = sum_n C[n,i] delta[n,j] is staged in LDS from the batch rows that
 *   rated i (ascending batch row) and Adam is applied; rows no batch user rated take the Adam update all the same (momentum).
 *   The bias is one more row, gb[j] = sum_n delta[n,j].  d_gradW_out [n_items][ld] / d_gradb_out [ld] (may be null) receive
 *   the gradient.
 * qrec_cfgan_read_slots: copies of r^, delta [n_live] and a_r, a_f [B] out of the workspace (each may be null).
 * Workspace: qrec_cfgan_workspace_bytes(B, n_live), shared by the calls of a step. */
#define QREC_CFGAN_CHUNK 1024
#define QREC_CFGAN_MAX_ITEMS 131072
int qrec_cfgan_workspace_bytes(int32_t B, int64_t n_live, int64_t *bytes);
int qrec_cfgan_forward(const float *d_W, const float *d_b, const float *d_thetaD, int32_t n_items, int32_t ld, int32_t B, int64_t n_in,
                       int64_t n_live, const int32_t *d_in_ptr, const int32_t *d_in_item, const float *d_in_val, const int32_t *d_lv_ptr,
                       const int32_t *d_lv_item, const int32_t *d_lv_flag, float alpha, void *d_ws, double *d_losses, void *stream);
int qrec_cfgan_dis_step(float *d_thetaD, float *d_mD, float *d_vD, int32_t n_items, int32_t B, int64_t n_in, int64_t n_live,
                        const int32_t *d_in_cptr, const int32_t *d_in_crow, const float *d_in_cval, const int32_t *d_lv_cptr,
                        const int32_t *d_lv_crow, const int32_t *d_lv_cslot, void *d_ws, float adam_alpha, float beta1, float beta2, float eps,
                        float *d_grad_out, void *stream);
int qrec_cfgan_gen_sweep(float *d_W, float *d_mW, float *d_vW, float *d_b, float *d_mb, float *d_vb, int32_t n_items, int32_t ld, int32_t B,
                         int64_t n_in, int64_t n_live, const int32_t *d_in_cptr, const int32_t *d_in_crow, const float *d_in_cval,
                         const int32_t *d_lv_ptr, const int32_t *d_lv_item, const int32_t *d_lv_cptr, const int32_t *d_lv_cslot, void *d_ws,
                         float adam_alpha, float beta1, float beta2, float eps, float *d_gradW_out, float *d_gradb_out, void *stream);
int qrec_cfgan_read_slots(const void *d_ws, int32_t B, int64_t n_live, float *d_rhat, float *d_delta, float *d_a_r, float *d_a_f, void *stream);
/* qrec_score_topk's BLOCK route for CFGAN's evaluation (CFGAN.py:129-134): the score block is FILLED from the rated CSR with
 * values (d_rated_indptr int64 [n_users + 1], rows ascending), S[item][b] = sum over the rated i of user b, ascending i, of
 * C[u,i] d_W[i][item] -- no users x items input is formed -- then sigmoid(S + d_item_bias[item]), rated items to 0, top-N. */
int qrec_score_topk_sparse_row_sigmoid_bias_scratch_bytes(int32_t n_items, int32_t n_batch_users, int64_t *bytes);
int qrec_score_topk_sparse_row_sigmoid_bias(const float *d_W, const float *d_item_bias, int32_t ld, int32_t n_items,
                                            const int32_t *d_user_ids, int32_t n_batch_users, const int64_t *d_rated_indptr,
                                            const int32_t *d_rated_items, const float *d_rated_vals, int32_t N, void *d_scratch,
                                            int32_t *d_ids_out, float *d_scores_out, void *stream);

/* ---- APR (model/ranking/APR.py; csrc/apr.hip), fp32.  d_E = the joint [U; V] table ([n_rows][ld], item row = n_users + item,
 * ld in {32, 64, 128}, d live columns, pad columns zero), d_D = the perturbations in the same layout.  For a triplet (u, i, j):
 * x = p_u.(q_i - q_j), x' = (p_u+D_u).((q_i+D_i) - (q_j+D_j)), g = -sigma(-x), c' = -reg_adv sigma(-x').
 *
 * qrec_apr_perturb (APR.py:43-53, one Session.run of update_U and update_V on the feeds u, v, n): on return every row of d_D that
 * this batch does not touch is zero and every touched row is eps * Gamma * rsqrt(max(|Gamma|^2, 1e-12)) (tf.nn.l2_normalize over the
 * d live columns), Gamma being the gradient of reg_adv sum softplus(-x') w.r.t. D, read with d_D as the previous call left it:
 *   user row:  sum over its u slots, ascending, of c' ((q_v+D_v) - (q_n+D_n))
 *   item row:  (sum over its v slots of c' (p_u+D_u)) + (sum over its n slots of -c' (p_u+D_u)), each lookup's slots ascending first.
 * With d_v == d_n elementwise every Gamma row is +-0 and d_D comes out exactly +0.  No float atomics: producer, one stable
 * radix sort of (row, slot), one walk that adds, normalises and writes the row; same inputs, same bits.  Work per call is
 * proportional to B and to the previous call's B, never to n_rows: d_touched (int32 [1 + touched_capacity], ZERO before the
 * first call, kept by the caller between calls, touched_capacity >= 3 B) lists the rows the previous call wrote, which are
 * cleared first.  B = 0 clears them and returns.  An index outside its table gives that triplet no row.
 * Workspace: qrec_apr_perturb_workspace_bytes(B, ld).  h_stage_ms (HOST float[4], NULL in training): a measurement aid -- the call
 * then records events around its stages, waits for the last and writes the device milliseconds of producer, clear, sort, walk.
 *
 * qrec_apr_batch_loss_grad (APR.py:56-64): d_loss (double[3]) is ACCUMULATED into: sum softplus(-x); reg (l2_loss(p_u) + l2_loss(q_i));
 * reg_adv sum softplus(-x').  d_dE (pre-zeroed, [n_rows][ld]) receives
 *   dE[u] += g (q_i-q_j) + reg p_u + c' ((q_i+D_i)-(q_j+D_j));  dE[nu+i] += g p_u + reg q_i + c' (p_u+D_u);  dE[nu+j] += -g p_u - c' (p_u+D_u)
 * A null d_D or reg_adv = 0 is the pretraining step (no perturbed term, d_loss[2] untouched).  d_workspace NULL = throughput
 * mode: float atomics on 64-byte segments and one fp64 atomic per block and term; a workspace of
 * qrec_apr_step_workspace_bytes(B, ld) bytes = parity mode: every row's gradient is the sum of its lookups' slots in batch
 * order, one lookup (u, i, j) at a time (qrec_scatter_add_rows_ordered's rule), the loss sums folded in a fixed tree.
 * A triplet with an index outside its table contributes nothing. */
int qrec_apr_perturb_workspace_bytes(int32_t B, int32_t ld, int64_t *bytes);
int qrec_apr_perturb(const float *d_E, float *d_D, int32_t n_users, int64_t n_rows, int32_t d, int32_t ld, const int32_t *d_u,
                     const int32_t *d_v, const int32_t *d_n, int32_t B, float reg_adv, float eps, int32_t *d_touched,
                     int32_t touched_capacity, void *d_workspace, int64_t workspace_bytes, float *h_stage_ms, void *stream);
int qrec_apr_step_workspace_bytes(int32_t B, int32_t ld, int64_t *bytes);
int qrec_apr_batch_loss_grad(const float *d_E, const float *d_D, int32_t n_users, int64_t n_rows, int32_t d, int32_t ld,
                             const int32_t *d_u, const int32_t *d_i, const int32_t *d_j, int32_t B, float reg, float reg_adv,
                             float *d_dE, double *d_loss, void *d_workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QREC_HIP_H */
