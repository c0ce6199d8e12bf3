/*
 * filmyou.h -- C ABI of the MI355X-native replacement for filmyou-core's two recommendation jobs.
 *
 * This is the drop-in boundary: the entry points below are what a JNI shim binds in place of the reference's
 * MapReduce Driver/Mapper/Reducer classes (binding shown in INTEGRATION.md).  Plain pointers and sizes only.
 * M/ = src/main/java/es/udc/fi/dc/irlab/ in dvalcarce/filmyou-core.
 *
 *   fy_rm2_*      replaces  ToolRunner.run(conf, new RM2Job(), args)   M/rmrecommender/RMRecommenderDriver.java:200-201
 *                 i.e. M/rm/RM2Job.java:76-100 (jobs RM2-1, RM2-2, RM2-3) and everything they run:
 *                 the M/rm mappers, the M/rm DoubleSum reducers, M/rm/AbstractRM2Reducer.java:129-389,
 *                 M/common/AbstractByCluster*Mapper.java (routing), M/util/IntDouble.java (ordering).
 *   fy_itemsim_*  replaces  ToolRunner.run(getConf(), new RowSimilarityJob(), {...})
 *                 M/baselinerecommender/BaselineRecommenderJob.java:241-253 (Mahout 0.8 RowSimilarityJob).
 *
 * Conventions: no exceptions cross the ABI; every function returns FY_OK (0) or a negative fy_status and leaves a
 * message for fy_last_error() (thread-local).  Input arrays are caller-owned and may be freed as soon as the call
 * returns.  Results are library-owned until fy_result_free.  One fy_context drives one GPU; a process uses one
 * context per device (one process per GPU under torch.distributed / a Hadoop task per GPU).  A context is not
 * re-entrant: calls on one context must not overlap; distinct contexts may be used from distinct threads.
 * Every entry point that takes a context, or a ratings / job / result object made on one, selects that context's
 * device for the calling thread (hipSetDevice) before it touches the GPU, and leaves it selected: a host may drive
 * several devices from one process and hand an object to another thread.
 * There is NO CPU fallback: without a gfx950 device every compute entry point fails with FY_ERR_NO_DEVICE.
 */
#ifndef FILMYOU_H
#define FILMYOU_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FY_ABI_VERSION 5

typedef enum {
    FY_OK = 0,
    FY_ERR_INVALID_ARGUMENT = -1,
    FY_ERR_NO_DEVICE = -2,       /* no HIP device / not gfx950 */
    FY_ERR_HIP = -3,             /* a HIP runtime call failed */
    FY_ERR_OUT_OF_MEMORY = -4,
    FY_ERR_CLUSTER_RANGE = -5,   /* a user is routed to a cluster outside [0, numberOfClusters): the reference would
                                    throw ArrayIndexOutOfBounds at M/common/AbstractByClusterAndCountMapper.java:88 */
    FY_ERR_CLUSTER_COUNT = -6,   /* clusteringCount disagrees with the rated users routed to a cluster: the reference
                                    reducer reads exactly clusterSizes[c] user-sum records first (AbstractRM2Reducer.java:153-160) */
    FY_ERR_DUPLICATE_RATING = -7,/* two ratings for one (user, item): Cassandra's PRIMARY KEY (user, item) forbids it */
    FY_ERR_NEGATIVE_ID = -8,     /* user / item ids must be >= 0 */
    FY_ERR_STATE = -9,           /* calls made out of order */
    FY_ERR_UNSUPPORTED = -10,
    FY_ERR_COLLECTIVE = -11,     /* a fy_collectives callback returned non-zero */
    FY_ERR_IO = -12              /* fy_seqfile_* / fy_mapfile_*: missing, truncated, compressed or foreign-typed file */
} fy_status;

typedef struct fy_context fy_context;
typedef struct fy_ratings fy_ratings;
typedef struct fy_rm2_job fy_rm2_job;
typedef struct fy_result fy_result;

/* ------------------------------------------------------------------ context */
int fy_abi_version(void);
const char* fy_last_error(void);
/* Binds the calling process to GPU `device_ordinal`, creates the HIP stream every kernel of this context runs on. */
int fy_context_create(int device_ordinal, fy_context** out);
void fy_context_destroy(fy_context*);
int fy_context_synchronize(fy_context*);
/* Fault injection for the error-path tests (the reference has none): the nth HBM request of this
 * context from now on (1 = the next one) fails with FY_ERR_OUT_OF_MEMORY; 0 disarms.  A failed job leaves the context
 * usable: every stream is drained before any buffer of the job is released. */
int fy_context_inject_alloc_failure(fy_context*, int64_t nth);
/* The library's launch-shape knobs (FY_* environment variables: test and measurement hooks) are read from
 * the environment once, by fy_context_create; this call reads them again.  No job reads the environment. */
int fy_context_reload_tuning(fy_context*);
/* The hipStream_t of the context (as void*), e.g. to order caller-side copies against the job. */
void* fy_context_stream(fy_context*);

/* ------------------------------------------------------------------ ratings
 * COO triples with the caller's raw int32 ids (1-based in the reference's data) exactly as the reference's
 * mappers receive them: table ratings(user int, item int, score float) (test/.../util/CassandraUtils.java:93-94) or
 * SequenceFile<IntPairWritable(user,item), FloatWritable> (M/util/DataInitialization.java:164-172).
 * `location`: FY_HOST pointers are copied over PCIe; FY_DEVICE pointers (HBM of the context's GPU) are copied
 * device-to-device, so the caller keeps ownership either way.
 * Id range: every user and item id in [0, 2^31 - 1] is accepted (a negative id is FY_ERR_NEGATIVE_ID), sparse or dense; the
 * jobs depend on the ids through their order alone.  RM2, item similarity and item-based CF (full jobs and requests) size
 * nothing by the largest id, with two exceptions that only switch an optimisation off: RM2's refinement pass keeps a table of
 * (largest item id + 1) entries and runs only while that id is below 2^28, and the sharded multi-rank prep lays its exchange
 * buffer out by raw id and is used only while (largest user id + 1) + (largest item id + 1) <= 2^25.  fy_submap_create and
 * fy_cluster_refine DO size their tables by raw id (largest user id of ratings and map + 1 entries; numberOfClusters x (largest
 * item id + 1) entries): user id 2^31 - 1, or that product reaching 2^31, is FY_ERR_UNSUPPORTED.  fy_nmf_* takes ids in
 * [1, numberOfUsers] / [1, numberOfItems] by contract. */
enum { FY_HOST = 0, FY_DEVICE = 1 };
int fy_ratings_create(fy_context*, int64_t nnz, const int32_t* user, const int32_t* item, const float* score,
                      int location, fy_ratings** out);
void fy_ratings_destroy(fy_ratings*);
int64_t fy_ratings_nnz(const fy_ratings*);
/* Releases what the jobs keep on the ratings object between calls (see fy_rm2_params::flags): the next job builds everything again.
 * A caching job whose clustering, rank or world differs from the kept state's releases it itself before it builds its own; a
 * FY_RM2_NO_CACHE job neither uses nor touches it (call this first when its memory is wanted back: the kept state of an ML-25M-shaped
 * job is ~2.5 GB).  Jobs over ONE ratings object must not run concurrently; distinct ratings objects (and contexts) may. */
void fy_ratings_drop_cache(fy_ratings*);

/* Ratings that take writes.  The reference's table is ratings(user int, item int, score float, PRIMARY KEY (user, item)): in CQL a
 * write to an existing key replaces the row and a DELETE removes it.  fy_ratings_apply makes a NEW, independent ratings object from
 * `source` and a batch of n writes (user, item, score, remove) taken in order; the batch is resolved on the GPU (csrc/
 * fy_ratings_update.hip) and the source is neither uploaded again nor modified: what the jobs kept on it stays
 * valid, the new object starts with none.  `remove_or_null`: n bytes, NULL = no deletes; a non-zero byte makes that write a delete
 * of its key, whose score is ignored.
 *   1. Later writes to one (user, item) supersede earlier ones of the batch: only the LAST write per key counts -- the batch equals
 *      replaying it row by row against the table.
 *   2. Every entry of the source whose key appears anywhere in the batch is dropped, also when the key's last write is a delete;
 *      several source entries with that key are all dropped (a write cures an old duplicate).
 *   3. The result is the surviving source entries IN THEIR SOURCE ORDER, followed by the last writes that are not deletes, in the
 *      order of their positions in the batch.
 *   4. Scores are stored as given, exactly as fy_ratings_create stores them: a score <= 0 is a stored rating, not a delete (the RM2
 *      mappers' score > 0 filter and the item-CF ratingShift treat it as they do today); NaN and negative ids get nothing at this
 *      point, as in fy_ratings_create, and the jobs report what they report today.  Keys compare as 64 bits made of the two 32-bit
 *      patterns, so any id is a key.
 *   5. The id bounds kept with the new object are those of its own contents.
 *   6. An empty batch gives a copy; an empty source gives the batch resolved by rule 1.
 * `location` (FY_HOST / FY_DEVICE) says where user / item / score / remove_or_null live, as in fy_ratings_create; the arrays may be
 * freed when the call returns.  n > 2^31 - 1 is FY_ERR_UNSUPPORTED.  On any failure *out is NULL and the source is intact.
 * Counters (stats_or_null):
 *   n_writes          n
 *   n_superseded      writes that are not the last of their key
 *   n_replaced        last non-delete writes whose key was in the source
 *   n_inserted        last non-delete writes whose key was not in the source
 *   n_deleted         last deletes whose key was in the source
 *   n_delete_missed   last deletes whose key was not in the source
 *   n_source_dropped  source entries dropped (more than n_replaced + n_deleted only when the source held duplicates)
 *   nnz_out           entries of the result = nnz of the source - n_source_dropped + n_replaced + n_inserted */
typedef struct { int64_t n_writes, n_superseded, n_replaced, n_inserted, n_deleted, n_delete_missed,
                 n_source_dropped, nnz_out; } fy_ratings_update_stats;
int fy_ratings_apply(fy_context*, const fy_ratings* source, int64_t n, const int32_t* user, const int32_t* item,
                     const float* score, const uint8_t* remove_or_null, int location,
                     fy_ratings** out, fy_ratings_update_stats* stats_or_null);
/* The COO as it lives in HBM, copied to HOST arrays of fy_ratings_nnz entries each (synchronises the ratings' context). */
int fy_ratings_copy_out(const fy_ratings*, int32_t* user, int32_t* item, float* score);

/* ------------------------------------------------------------------ RM2 job
 * Field names follow the Hadoop Configuration keys of M/rmrecommender/RMRecommenderDriver.java:49-120. */
typedef struct {
    double lambda;                      /* "lambda" (default 0.1), Jelinek-Mercer smoothing; with a FY_RM2_SMOOTHING_* flag: that method's
                                           parameter ("mu" / "delta"), see below */
    int32_t number_of_items;            /* "numberOfItems": global item count, used only in pvpi (AbstractRM2Reducer.java:327-329) */
    int32_t number_of_recommendations;  /* "numberOfRecommendations" (default 1000) */
    int32_t filter_users;               /* "filterUsers": users with id < this get no list (AbstractRM2Reducer.java:221-223) */
    int32_t number_of_clusters;         /* "numberOfClusters" */
    int32_t rank;                       /* this process scores user shard `rank` of `world` (1 GPU: 0 of 1) */
    int32_t world;
    uint32_t flags;                     /* FY_RM2_* below, 0 = defaults */
    int64_t workspace_bytes;            /* cap for the per-batch score scratch in HBM; 0 = default (16 GiB) */
} fy_rm2_params;

/* flags: by default a job keeps what it built from the ratings and the clustering alone (CSR / CSC, per-item statistics, the row
 * kernel's tables) on the fy_ratings object, and a later job over the same ratings AND the same clustering (and rank / world)
 * starts from it -- fy_stats::prepared_from_cache / tables_from_cache.  The reference has no such state: every RM2Job.run re-reads
 * and re-shuffles the ratings (RM2Job.java:130-258).  FY_RM2_NO_CACHE: build everything in this job, keep nothing (the "cold" job). */
#define FY_RM2_NO_CACHE 1u
/* Smoothing of the user language model.  The reference has one estimator, c_vi = (1-l) r_vi / s_v + l p(i|C)
 * (probItemGivenUser, AbstractRM2Reducer.java:384-389: Jelinek-Mercer); the two other standard smoothings have the same shape
 *     c_vi = w * r'_vi / d_v + beta_v * p(i|C)
 *
 *   method                                   r'_vi              d_v        beta_v            w
 *   (no bit) Jelinek-Mercer, l in [0, 1]     r_vi               s_v        l                 1 - l
 *   FY_RM2_SMOOTHING_DIRICHLET, mu >= 0      r_vi               s_v + mu   mu / (s_v + mu)   1
 *   FY_RM2_SMOOTHING_ABSOLUTE_DISCOUNT,      max(r_vi - d, 0)   s_v        d * n_v / s_v     1
 *                          delta = d >= 0
 *
 * with s_v the user's rating sum and n_v the number of its kept ratings (score > 0).  The method's parameter travels in
 * fy_rm2_params::lambda: l (validated to [0, 1] as always), mu or delta (finite and >= 0); anything else, and both bits set, is
 * FY_ERR_INVALID_ARGUMENT.  Everything else about a job is the same for the three methods: the candidates of a user are the items
 * of its cluster it has not rated (under absolute discounting a rating <= delta is still a rated item: it is no candidate and
 * contributes a log term), the side outputs (userSum, itemColl, the total, quirk Q1) are those of the raw ratings, mu = 0 and
 * delta = 0 give -inf for a candidate never co-rated with a rated item as l = 0 does, and a one-user cluster gives -inf rows.
 * What a caching job keeps on the fy_ratings object depends on (method, parameter) for the two new methods -- a caching job with
 * another key releases the kept state and builds its own, as for another clustering -- and on nothing of the kind for
 * Jelinek-Mercer, whose jobs are bit for bit what they were before these flags existed.
 * A job that would score a cluster cooperatively (collectives installed, see fy_rm2_set_collectives) answers
 * FY_ERR_UNSUPPORTED from fy_rm2_score with either flag; the context stays usable. */
#define FY_RM2_SMOOTHING_DIRICHLET 2u
#define FY_RM2_SMOOTHING_ABSOLUTE_DISCOUNT 4u
/* The estimator.  Parapar et al. 2013 define two relevance models; the reference ships RM2 (a product over the user's items of a sum
 * over neighbours).  FY_RM2_ESTIMATOR_RM1 makes fy_rm2_score, fy_rm2_score_users and fy_rm2_run emit RM1 lists instead: with the user
 * model c_vi above (the same table, all three methods -- the flag combines with either smoothing flag) and U_c users in the cluster,
 *
 *     score(u, i) = -ln U_c + ln  sum_{v in V_c, v != u}  c_vi * prod_{j in rated(u)} c_vj
 *
 * i.e. p(i|R_u) ~ sum_v p(v) p(i|v) prod_j p(j|v) with p(v) = 1 / U_c (the U_c of RM2's n ln U_c, not U_c - 1).  Everything an RM2
 * job fixes stays: kept ratings are score > 0; s_v, n_v and p(i|C) with the counter quirk Q1; the routing (an unmapped user goes to
 * cluster 0); the neighbourhood V_c \ {u}; the candidates of u are the items of its cluster it has not rated; a user without a
 * candidate gets no list; filterUsers and numberOfRecommendations; the (float) cast, ties by ascending item id, users in the order of
 * the unrestricted job, the cluster column; the side outputs, which are those of the raw ratings.  Consequences:
 *   - numberOfItems plays no role (it is still validated);
 *   - a kept rating with r' = 0 under absolute discounting is still a rated item: no candidate, one factor beta_v p_j;
 *   - with beta_v = 0 (lambda = 0, mu = 0, delta = 0) a neighbour that has not rated every item of u has likelihood 0;
 *   - if every neighbour's likelihood is 0, or U_c = 1, every row of u is -inf;
 *   - a candidate none of the neighbours with positive likelihood gives mass to is -inf.
 * The pass is fp64 in front of the (float) cast and never forms a likelihood unshifted: with L_uv = sum_j ln c_vj and
 * m_u = max_v L_uv, score = -ln U_c + m_u + ln(sum_v exp(L_uv - m_u) c_vi) (csrc/fy_rm1.hip).  No
 * floating-point atomics and a fixed summation order: a row's bits do not depend on the run, the batch, the FY_RM1_* chunk widths,
 * or on whether it came from fy_rm2_score or fy_rm2_score_users.  Per batch of users the weights (B x U_c x 8 bytes) and the score
 * rows (B x I_c x 4 bytes) are capped by workspace_bytes; one user whose own rows do not fit fails with FY_ERR_OUT_OF_MEMORY and is
 * named.  Work: U_c x nnz_c row entries per product and cluster for a full job, nnz_c per requested user.
 * Ranks: (rank, world) cut the slots as for the general smoothings (replicated and sharded prep both work); a job that would
 * score a cluster cooperatively (collectives installed) answers FY_ERR_UNSUPPORTED from fy_rm2_score and the context stays usable.
 * FY_REQ_FULL_SHARE has no meaning under RM1: there is one pass.  Without the flag nothing about any job changes; what a caching
 * job keeps on the fy_ratings object does not depend on the flag.  Bits of flags outside the four FY_RM2_* are
 * FY_ERR_INVALID_ARGUMENT.
 * fy_result_stats of an RM1 result: users_scored, recs, pair_contribs = sum over the scored users u of (nnz_c - n_u) (entries of the
 * neighbours' rows tested against the user's rated set: the first product), log_terms = sum over the scored users of nnz_c (entries
 * of the cluster's columns gathered: the second product), cooc_launches / score_launches (= batches), ms_tables (e, ln p, a),
 * ms_cooc (likelihoods and weights), ms_score, ms_topn, ms_total; fy_result_request_stats of a request: users_asked, users_known,
 * clusters_touched, batches. */
#define FY_RM2_ESTIMATOR_RM1 0x8u

/* Stage 1 (jobs RM2-1/RM2-2 up to the exchange): score > 0 filter, CSR/CSC in HBM, cluster routing, user sums,
 * and this rank's PARTIAL per-item rating sums + partial floor-sum total.
 * Clustering = the reference's `clustering` file as (user, cluster) pairs; n_map = 0 routes every user to
 * cluster 0 (Trove default, quirk Q2).  cluster_count (numberOfClusters ints, the `clusteringCount` file) may be
 * NULL; when given it is validated.  map_* / cluster_count are HOST pointers. */
int fy_rm2_prepare(fy_context*, const fy_rm2_params*, const fy_ratings*, int64_t n_map, const int32_t* map_user,
                   const int32_t* map_cluster, const int32_t* cluster_count, fy_rm2_job** out);
/* The exchange buffer of this rank, in HBM: `*len` doubles, the same `*len` on every rank (the ratings are replicated):
 * all-gather it (RCCL) into world * len doubles.  Two layouts (fy_rm2_stats_layout tells which):
 *   replicated prep : [one partial rating sum per rated item, ascending raw item id][this rank's partial sum of floor(s_u), quirk Q1]
 *   sharded prep    : a job of several ranks with at least as many non-empty clusters as ranks gives every rank WHOLE clusters and
 *                     preps the ratings of its own clusters alone (the reference's map-side partitioning by cluster,
 *                     IntKeyPartitioner.java:15); its buffer is indexed by RAW id:
 *                     [max item id + 1 item sums][the floor-sum][max user id + 1 user sums s_u][failure flag of this rank's share]. */
int fy_rm2_partial_stats(fy_rm2_job*, double** device_buf, int64_t* len);
/* n_item_slots item sums, one floor-sum, n_user_slots user sums (0: replicated prep, no user sums and no flag), the flag. */
int fy_rm2_stats_layout(fy_rm2_job*, int64_t* n_item_slots, int64_t* n_user_slots);
/* `gathered` = world * len doubles in HBM, rank-major.  Summed in rank order (bit-reproducible).  Optional when world == 1. */
int fy_rm2_set_global_stats(fy_rm2_job*, const double* gathered_device, int32_t world);
/* Collectives of the process group the `world` ranks form (one process per GPU).  The signatures are RCCL's
 * (ncclAllGather / ncclReduceScatter with ncclSum on float): device pointers, the operation is enqueued in order on
 * `stream` (a hipStream_t) -- no host synchronisation is implied.  Return 0 on success.  `user` is handed back verbatim.
 *   all_gather:      recv[k * bytes .. (k + 1) * bytes) = rank k's send[0 .. bytes)
 *   reduce_scatter:  recv[i] = sum over ranks k of send_k[rank * count + i],  i < count   (send holds world * count floats)
 * With collectives installed, a cluster whose users span ALL ranks is scored cooperatively: every rank
 * builds only its row range of the cluster's co-rating matrix, evaluates every user's partial log-sums over those rows, and
 * the partial sums of the seed columns, of the block bounds and of the surviving blocks are reduce-scattered to the rank
 * that owns the user -- about 1/world of the single-GPU work and matrix per rank.  Without them (or when a cluster lives on
 * fewer ranks) every rank builds the whole matrix of the clusters it holds users of, and only the user loop is sharded.
 * If fy_rm2_set_global_stats was not called, fy_rm2_score all-gathers the partial statistics through `all_gather` itself.
 * Every rank must install collectives (or none), and all ranks must call fy_rm2_score together. */
typedef struct {
    void* user;
    int (*all_gather)(void* user, const void* send, void* recv, int64_t bytes, void* stream);
    int (*reduce_scatter_f32)(void* user, const float* send, float* recv, int64_t count, void* stream);
} fy_collectives;
int fy_rm2_set_collectives(fy_rm2_job*, const fy_collectives*);

/* The compiled transport for fy_collectives: RCCL (ncclAllGather / ncclReduceScatter over xGMI) queued on the context's own
 * stream, no host synchronisation.  librccl.so is opened at run time, a single-GPU host does not need it.  One process per
 * GPU: rank 0 makes the 128-byte id (fy_rccl_unique_id) and hands it to the other ranks by whatever channel the host has
 * (the Hadoop Configuration / a file / torch.distributed's store); fy_rccl_create is collective over all ranks
 * (ncclCommInitRank).  Replaces the shuffle + DistributedCache + counter exchange of M/rm/RM2Job.java:130-149, 184-198,
 * 260-263 for hosts that are not Python (the C++ mirror, the JNI shim). */
typedef struct fy_rccl fy_rccl;
int fy_rccl_unique_id(char* out128);
int fy_rccl_create(fy_context*, int rank, int world, const char* id128, fy_rccl** out);
int fy_rccl_collectives(fy_rccl*, fy_collectives* out);   /* fills the callbacks; `out->user` is the fy_rccl, which must outlive the job */
int fy_rccl_counters(const fy_rccl*, int64_t* all_gathers, int64_t* reduce_scatters, int64_t* payload_bytes);
void fy_rccl_destroy(fy_rccl*);           /* the context must still exist (its stream is drained first) ... */
void fy_rccl_detach_context(fy_rccl*);    /* ... unless this was called: the context is already gone, only the communicator is released */
/* Stage 2 (job RM2-3): per-cluster co-rating matrix, p(i|u) scoring of this rank's users, top-N. */
int fy_rm2_score(fy_rm2_job*, fy_result** out);
void fy_rm2_job_destroy(fy_rm2_job*);

/* RM2 on request: the lists of the named users alone ("these users just rated something"), with the work sized by the request.
 * Works on a prepared job whose global statistics are in place (after fy_rm2_set_global_stats, or world == 1); may be called any
 * number of times on one job, before or after fy_rm2_score, and leaves the job as it was.  The result holds exactly the rows
 * fy_rm2_score of the same job would emit for the listed users: filterUsers, "no candidate left -> no list",
 * numberOfRecommendations, the (float) cast, -inf at lambda = 0 or U_c = 1, the cluster column, ties by ascending item id, users in
 * the order of the unrestricted job, best first.  `users`: HOST array of raw ids in any order; a duplicate counts once; an id
 * without a kept rating, an id outside the data and a negative id are passed over without an error; n_users == 0 gives an empty
 * result; users == NULL with n_users > 0 is FY_ERR_INVALID_ARGUMENT.  (rank, world) of the job shard the requested users as they
 * shard the full job's users (replicated and sharded prep).  A job with collectives installed answers FY_ERR_UNSUPPORTED.
 * Per cluster that holds a requested user only the rows G[j][.] of the co-rating matrix with j rated by a requested user are
 * formed -- an fp64 slab in HBM, bit-reproducible, at most fy_rm2_params::workspace_bytes at a time (the users of a cluster are
 * taken in batches; one user whose own rows do not fit fails with FY_ERR_OUT_OF_MEMORY) -- and the whole pass is fp64 (DESIGN.md
 * section 2b).  A cluster of which more than FY_REQ_FULL_SHARE of the users is asked for (default: never) is scored by the full pass instead,
 * which runs the rank's whole full job once (full_pass_clusters).
 * fy_result_stats of the result: users_scored, recs, log_terms (of the requested users), pair_contribs (products the slab kernel
 * accumulated), cooc_matrix_bytes (slab bytes written), ms_tables, ms_cooc, ms_score, ms_topn, ms_total. */
typedef struct { int64_t n_users; const int32_t* users; } fy_rm2_request;   /* HOST, raw ids, any order */
int fy_rm2_score_users(fy_rm2_job*, const fy_rm2_request*, fy_result** out);
typedef struct {
    int64_t users_asked;         /* n_users of the request */
    int64_t users_known;         /* distinct requested users with a kept rating that this rank emits lists for */
    int64_t clusters_touched;    /* clusters that hold one of them */
    int64_t batches;             /* slabs built */
    int64_t slab_rows;           /* rows of all slabs (sum over the batches of |J|) */
    int64_t slab_bytes_peak;     /* largest slab */
    int64_t slab_pair_contribs;  /* sum over the slab rows j of sum over the raters v of j of n_v */
    int64_t full_pass_clusters;  /* touched clusters scored by the full pass with the unrequested rows dropped */
} fy_rm2_request_stats;
int fy_result_request_stats(fy_result*, fy_rm2_request_stats* out);          /* FY_ERR_STATE on any other result */

/* One call = one complete single-GPU job on host buffers (what the JNI shim calls): context on device 0. */
int fy_rm2_run(const fy_rm2_params*, int64_t nnz, const int32_t* user, const int32_t* item, const float* score,
               int64_t n_map, const int32_t* map_user, const int32_t* map_cluster, const int32_t* cluster_count,
               fy_result** out);

/* ------------------------------------------------------------------ item-item similarity build */
/* The seven measures Mahout 0.8's RowSimilarityJob accepts as --similarityClassname.  After the input preparation below, let
 * r_ui be the kept preferences, n_i the number of users with a preference for item i, N the number of distinct users that still
 * have a preference (what the reference passes as --numberOfColumns), and d = sum_u w_ui w_uj over a pair (i, j) that AT LEAST ONE
 * USER CO-RATED (other pairs have no similarity):
 *
 *   constant                          column transform w_ui                    norm a_i      similarity
 *   FY_SIMILARITY_COSINE              r_ui / ||r_.i||_2                        -             d
 *   FY_SIMILARITY_COOCCURRENCE        1                                        -             d
 *   FY_SIMILARITY_TANIMOTO_COEFFICIENT 1                                       n_i           d / (a_i + a_j - d)
 *   FY_SIMILARITY_LOGLIKELIHOOD       1                                        n_i           1 - 1 / (1 + LLR(k11 = d, k12 = a_j - d, k21 = a_i - d,
 *                                                                                                           k22 = N - a_i - a_j + d))
 *   FY_SIMILARITY_CITY_BLOCK          1                                        n_i           1 / (1 + a_i + a_j - 2 d)
 *   FY_SIMILARITY_EUCLIDEAN_DISTANCE  r_ui                                     sum_u r_ui^2  1 / (1 + sqrt(max(0, a_i - 2 d + a_j)))
 *   FY_SIMILARITY_PEARSON_CORRELATION c_ui / ||c_.i||_2,                       -             d
 *                                     c_ui = r_ui - (sum_u |r_ui|) / n_i over the item's raters
 *
 * LLR(k11, k12, k21, k22) = 0 if rowE + colE < matE, else 2 (rowE + colE - matE), with H(x...) = xlogx(sum x) - sum xlogx(x),
 * xlogx(0) = 0, xlogx(x) = x ln x, rowE = H(k11 + k12, k21 + k22), colE = H(k11 + k21, k12 + k22), matE = H(k11, k12, k21, k22).
 * The finishing arithmetic is fp64; the emitted value is its (float).  Kept: j != i when exclude_self, sim >= threshold (no
 * threshold: sim > 0), the max_similarities_per_item best per item, ties by ascending item id.  A NaN similarity (Pearson of an
 * item whose raters all gave the same rating) is dropped.  Mahout's consider() pre-pruning and its random down-sampling are not
 * modelled.  "Co-rated" is decided by d != 0, which is exact for the count measures and wherever every preference is positive:
 *   - FY_SIMILARITY_EUCLIDEAN_DISTANCE on data with a non-positive preference fails with FY_ERR_UNSUPPORTED;
 *   - FY_SIMILARITY_PEARSON_CORRELATION with has_threshold and threshold <= 0 fails with FY_ERR_UNSUPPORTED (a co-rated pair whose
 *     centred products cancel to 0 cannot be told from a pair nobody co-rated).
 * A Pearson item counts as constant only where ||c_.i|| is exactly 0, i.e. where (sum |r|) / n_i reproduces the common rating bit
 * for bit in fp64 -- true for integers and half steps; for ratings such as 0.1f with n_i not a power of two the centred values
 * are rounding residue, the item keeps weights made of it and its similarities mean nothing (as in any fp64 evaluation of the
 * definition).
 * Pearson's weights are fp32 (absolute error of a similarity <= 2^-23); where the preferences are not exactly representable in
 * fp16 the Euclidean dot product is an fp64 sum in the order the atomics land, and a_i - 2 d + a_j of two nearly identical columns
 * cancels. */
enum {
    FY_SIMILARITY_COSINE = 0,
    FY_SIMILARITY_COOCCURRENCE = 1,
    FY_SIMILARITY_TANIMOTO_COEFFICIENT = 2,
    FY_SIMILARITY_LOGLIKELIHOOD = 3,
    FY_SIMILARITY_CITY_BLOCK = 4,
    FY_SIMILARITY_EUCLIDEAN_DISTANCE = 5,
    FY_SIMILARITY_PEARSON_CORRELATION = 6
};
typedef struct {
    int32_t similarity;                 /* --similarityClassname: one of FY_SIMILARITY_* */
    int32_t max_similarities_per_item;  /* --maxSimilaritiesPerRow (default 100, BaselineRecommenderJob.java:67) */
    int32_t exclude_self;               /* --excludeSelfSimilarity (call site passes true) */
    int32_t has_threshold;              /* 0 = RowSimilarityJob.NO_THRESHOLD */
    double threshold;                   /* --threshold */
    int32_t rank;                       /* this process builds item-row shard `rank` of `world` */
    int32_t world;
    uint32_t flags;
    /* input preparation of the preference matrix (M/baselinerecommender/BaselinePreparePreferenceMatrixJob.java:104, 126-129):
     * users with fewer than min_prefs_per_user preferences are dropped (Mahout ToUserVectorsReducer.MIN_PREFERENCES_PER_USER;
     * reference default 1 = nobody); users with more than max_prefs_per_user preferences are cut down to that many.  Mahout's
     * ToItemVectorsMapper draws a RANDOM sample there (no reproducible output exists), this library a DETERMINISTIC systematic
     * one over the user's preferences in ascending item id: preference k of n is kept iff floor((k+1) m / n) > floor(k m / n)
     * -- NOT parity with any particular Mahout run, documented as such.  0 = option off. */
    int32_t min_prefs_per_user;
    int32_t max_prefs_per_user;
} fy_itemsim_params;
int fy_itemsim_build(fy_context*, const fy_itemsim_params*, const fy_ratings*, fy_result** out);
int fy_itemsim_run(const fy_itemsim_params*, int64_t nnz, const int32_t* user, const int32_t* item,
                   const float* score, fy_result** out);

/* ------------------------------------------------------------------ item similarity on request: the rows of named items
 * "Items similar to this one" (Mahout's ItemBasedRecommender.mostSimilarItems) is one row of the similarity matrix.
 * fy_itemsim_prepare builds, once per ratings object, everything the similarity job derives from the ratings and the parameters
 * alone (O(nnz)): it validates exactly what fy_itemsim_build validates (same codes, same messages), applies the input
 * preparation, builds the CSR / CSC, the per-item norms / counts / sum r^2 / Pearson centres (fixed summation order) and the row
 * offsets of the request kernel's column chunks.  The job owns its buffers; the ratings may be destroyed after prepare.  A job
 * over an empty preference matrix is valid and answers every request with an empty result.  To follow a write, prepare again on
 * the new ratings object (fy_ratings_apply).
 * fy_itemsim_rows answers any number of requests and leaves the job as it was.  The result (a similarity result like
 * fy_itemsim_build's) holds exactly the rows fy_itemsim_build with the same parameters would emit for the listed items: the
 * full build's item order (popularity rank), within a row best first, ties by ascending raw item id, exclude_self,
 * sim >= threshold / sim > 0, NaN dropped, the max_similarities_per_item best.  `items`: HOST array of raw ids in any order; a
 * duplicate counts once; an id nobody rated, an id outside the data, a negative id and an item lost to the input preparation are
 * passed over without an error; n_items == 0 gives an empty result; items == NULL with n_items > 0 is
 * FY_ERR_INVALID_ARGUMENT.  (rank, world) of the parameters: a rank answers only for the requested items whose row its full
 * build would own (popularity rank % world == rank).
 * Work: sum over the requested items j of sum over the raters v of j of n_v products; nothing in a request runs over all
 * ratings or all users.  Values: the dot product d of a pair is accumulated in 64-bit fixed point (scale per row from a bound
 * of the row's entries; signed contributions add modulo 2^64), so it does not depend on the order of the atomics and two runs
 * give the same bits; it is exact whenever every product is a multiple of the grid and the sum fits -- half stars, integers,
 * the count measures.  The weights are the raw preference (cosine, Euclidean distance), 1 (the count measures) or the centred,
 * normalised preference in fp64 (Pearson); the finish is the full build's fp64 arithmetic.  On half-star or integer preferences
 * the rows are bitwise the full build's for every measure but Pearson; Pearson, and cosine on preferences that are not
 * fp16-exact, differ from the full build (whose weights are fp32 there) within the bounds stated above.
 * fy_result_stats of a request result: n_users (N after the input preparation), n_items, nnz, recs, pair_contribs (below),
 * cooc_launches (= batches), ms_prepare = 0, ms_cooc (row kernel), ms_topn (merge + compaction), ms_total. */
typedef struct fy_itemsim_job fy_itemsim_job;
int fy_itemsim_prepare(fy_context*, const fy_itemsim_params*, const fy_ratings*, fy_itemsim_job** out);
void fy_itemsim_job_destroy(fy_itemsim_job*);
typedef struct { int64_t n_items; const int32_t* items; } fy_itemsim_request;   /* HOST, raw item ids, any order */
int fy_itemsim_rows(fy_itemsim_job*, const fy_itemsim_request*, fy_result** out);
typedef struct {
    int64_t items_asked;      /* n_items of the request */
    int64_t items_known;      /* distinct requested items with a kept preference that this rank answers for */
    int64_t rows_emitted;     /* of those, the items whose row is not empty */
    int64_t batches;          /* launches of the row kernel */
    int64_t pair_contribs;    /* sum over the known items j of sum over the raters v of j of n_v */
    int64_t chunks;           /* column chunks per row */
} fy_itemsim_request_stats;
int fy_result_itemsim_request_stats(fy_result*, fy_itemsim_request_stats* out);   /* FY_ERR_STATE on any other result */

/* ------------------------------------------------------------------ item-based CF recommendation (phases 3-4)
 * Replaces the partialMultiply and aggregateAndRecommend jobs of M/baselinerecommender/BaselineRecommenderJob.java:285-328,
 * 340-393 (reducer M/baselinerecommender/BaselineAggregateAndRecommendReducer.java:97-161, 195-235): prediction(u, i) =
 * sum_j sim(j, i) pref(u, j) / sum_j |sim(j, i)| over the user's maxPrefsPerUser strongest preferences j whose similarity
 * row holds i, kept only where at least two preferences contribute; items of those preferences are excluded; the
 * numRecommendations largest predictions per user.  `similarities` is the result of fy_itemsim_build with world == 1 on
 * the same context (the whole matrix).  Users are sharded by (rank, world).  Output rows: (user, item, (float) prediction, 0). */
typedef struct {
    int32_t num_recommendations;   /* --numRecommendations (default 100, BaselineRecommenderJob.java:66) */
    int32_t max_prefs_per_user;    /* --maxPrefsPerUser (default 50, :70) */
    int32_t boolean_data;          /* --booleanData */
    int32_t rank;
    int32_t world;
    uint32_t flags;
} fy_itemcf_params;
int fy_itemcf_recommend(fy_context*, const fy_itemcf_params*, const fy_ratings*, fy_result* similarities, fy_result** out);

/* ------------------------------------------------------------------ item-based CF: usersFile, itemsFile, ratingShift, item pairs
 * The remaining options of the job around the two calls above (M/baselinerecommender/BaselineRecommenderJob.java).
 *
 * usersFile (BaselineRecommenderJob.java:74, 189, 305-307; Mahout's UserVectorSplitterMapper passes over every user that is not
 * listed) and itemsFile (BaselineAggregateAndRecommendReducer.java:61, 170-181: itemsToRecommendFor; :209: only a listed item
 * enters the top-N queue).  has_* = 0 is the reference's NULL file name: the option is off.  The id arrays are HOST arrays of raw
 * ids in any order; a duplicate counts once; a user without a kept preference, an id outside the data and an item nobody rated
 * are passed over without an error; an option that is on with an empty list gives an empty result (Mahout's empty id set).
 * A user's list is the numRecommendations best predictions AMONG THE ALLOWED ITEMS (the allow-list is applied where a cell
 * becomes a prediction, not to the finished list); everything else -- the user's own items excluded, at least two contributing
 * preferences, NaN, the arithmetic, the 2048 limit, the row order (users in the order of the unrestricted job, best first) -- is
 * fy_itemcf_recommend's, and with both options off the call IS fy_itemcf_recommend.  (rank, world) shard the requested users.
 * The dense accumulators are sized by the users asked for.  fy_result_stats: users_scored = users that received a list, recs,
 * ms_prepare (structure of the ratings), ms_tables (similarity rows by column + the request's list and bitmap), ms_score
 * (accumulate + predictions), ms_topn, ms_total. */
typedef struct {
    int32_t has_users;  int32_t has_items;       /* 0 = option not given (NULL file in the reference) */
    int64_t n_users;    const int32_t* users;    /* HOST, raw user ids, any order, duplicates allowed */
    int64_t n_items;    const int32_t* items;    /* HOST, raw item ids */
} fy_itemcf_filter;
int fy_itemcf_recommend_filtered(fy_context*, const fy_itemcf_params*, const fy_itemcf_filter*,
                                 const fy_ratings*, fy_result* similarities, fy_result** out);
/* ------------------------------------------------------------------ item-based CF on request from a prepared similarity job
 * fy_itemcf_recommend_prepared is fy_itemcf_recommend_filtered without the similarity matrix as an input: a user's prediction needs
 * only the similarity rows of that user's own max_prefs_per_user strongest preferences, and the prepared job builds any row on
 * request.  The result holds exactly the rows fy_itemcf_recommend_filtered would emit with the same fy_itemcf_params, the same
 * filter, the ratings the job was prepared on and a similarity matrix whose rows are those fy_itemsim_rows of this job returns:
 * the user order (slot order of the unrestricted job), best first, ties at the cut, the strongest max_prefs_per_user preferences
 * with ties at the cut kept, the (j, NaN) self entry, at least two contributing preferences, the numerator == 0 skip,
 * boolean_data, the allow-list applied where a cell becomes a prediction, the 2048 limit, and (rank, world) of fy_itemcf_params
 * cutting the list of known requested users -- all bit for bit: the per-cell order of additions is still the order of the user's
 * preferences.  On half-star or integer preferences, for every measure but Pearson, fy_itemsim_rows is bitwise the full build and
 * the result is bitwise fy_itemcf_recommend_filtered's on the full matrix; for Pearson, and for cosine on preferences that are not
 * fp16-exact, it is the filtered pass fed with the job's own rows.
 * The filter must name users: filter == NULL or has_users == 0 is FY_ERR_INVALID_ARGUMENT (lists for everybody are
 * fy_itemcf_recommend's).  has_users with n_users == 0, has_items with n_items == 0, and a job over an empty preference matrix give
 * an empty result; unknown ids, negative ids and duplicates are passed over.  A job prepared with world != 1 (every rank needs any
 * row) or with min_prefs_per_user > 1 or max_prefs_per_user != 0 (its CSR is no longer the users' preference vectors) answers
 * FY_ERR_UNSUPPORTED.
 * The row store: rows built by a call stay on the JOB (not on the ratings) for later calls -- per column a state, a count, and
 * K = max_similarities_per_item entries (the other item as a popularity-rank column, the similarity): 8 K + 12 bytes per rated
 * item, allocated by the first call (FY_ERR_OUT_OF_MEMORY like any allocation).  A row is marked present only after it is
 * complete, so a call that fails half way leaves the job answering correctly.  The store changes no result: a cold job, a warm job
 * and a job after fy_itemsim_job_drop_rows (releases the store; the job stays valid) return the same bits.  There is no eviction,
 * and the store does not follow a write: prepare again on the new ratings.  fy_itemsim_rows neither reads nor fills it.
 * Work: sum over the rows BUILT of the row's walk (fy_itemsim_rows), plus the filtered pass's accumulate; nothing runs over all
 * ratings or all users, the dense accumulators are sized by the request.
 * fy_result_stats: nnz, n_users, n_items (the job's), users_scored = users that received a list, recs, pair_contribs,
 * cooc_launches (= batches), score_launches, ms_prepare = 0, ms_tables (request list, thresholds, the set J), ms_cooc (row kernel,
 * merge, store fill), ms_score, ms_topn, ms_total. */
typedef struct {
    int64_t users_asked;      /* n_users of the filter */
    int64_t users_known;      /* distinct requested users with a kept preference that this rank emits for */
    int64_t items_needed;     /* |J|: distinct items among the kept (strongest) preferences of those users */
    int64_t rows_built;       /* rows of J the row kernel had to build in this call */
    int64_t rows_from_store;  /* rows of J found in the job's row store */
    int64_t rows_stored;      /* rows in the store when the call returns */
    int64_t pair_contribs;    /* sum over the rows BUILT of sum over the raters v of the row's item of n_v */
    int64_t batches;          /* launches of the row kernel */
} fy_itemcf_request_stats;
int fy_itemcf_recommend_prepared(fy_itemsim_job*, const fy_itemcf_params*, const fy_itemcf_filter*, fy_result** out);
int fy_result_itemcf_request_stats(fy_result*, fy_itemcf_request_stats* out);   /* FY_ERR_STATE on any other result */
void fy_itemsim_job_drop_rows(fy_itemsim_job*);                                  /* releases the row store; the job stays valid */
/* ratingShift (BaselinePreparePreferenceMatrixJob.java:105-106, 201, 223; BaselineToItemPrefsMapper.java:51, 60): a NEW ratings
 * object whose scores are (float)(score + shift), added in fp32 like the mapper's `float prefValue`; ids as they are.  Nothing
 * the jobs kept on the source object is carried over.  The baseline job feeds it to the similarity build and to the
 * recommendation pass alike; shifted preferences may be non-positive, and what the similarity build does with such data holds
 * (FY_ERR_UNSUPPORTED for FY_SIMILARITY_EUCLIDEAN_DISTANCE). */
int fy_ratings_shifted(fy_context*, const fy_ratings*, float shift, fy_ratings** out);
/* outputPathForSimilarityMatrix (BaselineRecommenderJob.java:259-278: Mahout 0.8's ItemSimilarityJob.MostSimilarItemPairsMapper /
 * Reducer into a TextOutputFormat).  Those classes are third-party and restated from memory, as every Mahout class in this
 * package: PARITY UNPINNED.  `similarities` = the rows of a world == 1 fy_itemsim_build.  Result rows (key0 = min id, key1 = max id,
 * value = similarity, aux = 0): every unordered pair that occurs in at least one of the two items' rows, once, sorted by
 * (min, max); where both rows hold the pair the value is the one in the row of the smaller id.
 * fy_simpairs_write_text writes `a<TAB>b<TAB>sim` lines, sim = the shortest decimal (%.{1..17}g) that reads back as the float
 * widened to double; byte-for-byte agreement with Java's Double.toString is NOT claimed.  Host-only. */
int fy_itemsim_pairs(fy_context*, fy_result* similarities, fy_result** out);
int fy_simpairs_write_text(const char* file, int64_t n, const int32_t* a, const int32_t* b, const float* sim);

/* ------------------------------------------------------------------ cluster assignment (the stage in front of the RM2 job)
 * Replaces ClusterAssignmentJob's map-only jobs and CountClustersJob (M/nmf/clustering/ClusterAssignmentJob.java:60-135,
 * FindClusterMapper.java:37-45, FindSubClusterMapper.java:46-76, CountReducer.java:31-45): for every row j of H (n_rows x k
 * doubles, row-major; the factor matrix the NMF/PPC stage leaves behind)
 *     user[j] = first_user + j          (the SequenceFile key of DataInitialization.createDoubleMatrix / the H files)
 *     cluster[j] = cluster_offset + first index of the largest value of the row   (Vector.maxValueIndex(); -1 + no offset if
 *                  no value exceeds -infinity)
 * Sub-clustering calls it once per parent cluster c with cluster_offset = c * ceil(numberOfUsers / numberOfClusters).
 * count_inout (host, n_clusters ints, may be NULL) is INCREMENTED per routed user = the `clusteringCount` file; a cluster id
 * outside [0, n_clusters) then fails with FY_ERR_CLUSTER_RANGE.  H: FY_HOST or FY_DEVICE; user_out / cluster_out: host arrays of
 * n_rows ints -- exactly the (map_user, map_cluster, cluster_count) arguments of fy_rm2_prepare / fy_rm2_run. */
int fy_cluster_assign(fy_context*, int32_t n_rows, int32_t k, const double* H, int location, int32_t first_user,
                      int32_t cluster_offset, int32_t n_clusters, int32_t* user_out, int32_t* cluster_out, int32_t* count_inout);

/* ------------------------------------------------------------------ results
 * Rows as the reference writes them: RM2 (user, item, (float) relevance, cluster) -- RM2HDFSReducer.java:48 /
 * RM2CassandraReducer.java:49-63 -- grouped by user, best first; item-sim (item, other item, similarity) grouped by
 * item, best first.  Accessors return HOST pointers (the first accessor call downloads from HBM and synchronises). */
int64_t fy_result_size(fy_result*);
const int32_t* fy_result_key0(fy_result*);      /* user (RM2) | item (item-sim) */
const int32_t* fy_result_key1(fy_result*);      /* item (RM2) | other item (item-sim) */
const float* fy_result_value(fy_result*);       /* relevance | similarity */
const int32_t* fy_result_aux(fy_result*);       /* cluster (RM2) | 0 */
/* rm2/userSum and rm2/itemColl (what TestHDFSRM2.java:70-71 asserts), ascending raw id; RM2 only */
int64_t fy_result_n_users(fy_result*);
const int32_t* fy_result_user_id(fy_result*);
const double* fy_result_user_sum(fy_result*);
int64_t fy_result_n_items(fy_result*);
const int32_t* fy_result_item_id(fy_result*);
const double* fy_result_item_coll(fy_result*);
double fy_result_total_sum(fy_result*);
void fy_result_free(fy_result*);

typedef struct {
    int64_t nnz;               /* ratings kept (score > 0) */
    int64_t n_users, n_items, n_clusters_nonempty;
    int64_t users_scored;      /* users that received a list (this rank) */
    int64_t recs;              /* rows in the result (this rank) */
    int64_t log_terms;         /* RM2: (u, i unrated, j rated) terms evaluated by the scoring kernel (this rank) */
    int64_t pair_contribs;     /* ordered co-rating pair contributions accumulated by the row kernel (= sum n_u^2 walked) */
    int64_t unordered_pairs;   /* item-sim unit: sum_u n_u (n_u - 1) / 2 over the rows this rank builds */
    double ms_prepare;         /* HIP-event milliseconds on the context's stream, per phase */
    double ms_cooc;            /* co-rating row kernel (RM2: dense M build; item-sim: whole build) */
    double ms_score;           /* RM2 scoring kernel, summed over launches */
    double ms_topn;
    double ms_total;
    int64_t score_launches;    /* launches of the scoring kernels */
    int64_t cooc_launches;
    int64_t blocks_total;        /* RM2 branch and bound: (user, 256-column block) pairs behind the seed columns ... */
    int64_t blocks_survived;     /* ... and how many of them had to be scored exactly */
    int64_t log_terms_evaluated; /* log terms actually evaluated (seed + bound + survivor passes); 0 = no pruning: log_terms */
    int64_t prune_fallbacks;     /* user batches whose bound did not bite (e.g. lambda = 0) and that were redone with the full pass */
    double ms_tables;            /* RM2: p(i|C), per-rating values, packed CSR, chunk offsets and segment tables (between prepare and the M build) */
    double ms_mirror;            /* RM2: mirror pass of the symmetric walk (lower triangle of the co-rating matrix + its block maxima) */
    int64_t topn_select_users;   /* users whose list needed the radix-select fallback of the top-N kernel (more than 2048 candidates reached the lower bound) */
    int64_t panel_clusters;      /* clusters built in column-panel mode (many clusters: only the popular columns of the co-rating matrix are stored) */
    int64_t stray_blocks;        /* panel mode: surviving (user, block) pairs behind the panel, scored exactly from the sparse data */
    int64_t bound_repairs;       /* panel mode: 64-column sub-blocks dropped by the second bound (without the user's own co-ratings) */
    int64_t isim_candidates;     /* item similarity, symmetric build: candidates the band sweep appended to the rows' lists (of I^2 / 2 elements x 2 rows) */
    int64_t isim_redone_rows;    /* ... rows whose list overflowed and were redone exactly from the matrix */
    int64_t prepared_from_cache; /* RM2: 1 = fy_rm2_prepare found its structures on the fy_ratings object (same clustering): nothing was sorted */
    int64_t tables_from_cache;   /* RM2: 1 = the row kernel's tables (packed CSR, segment tables) were re-used */
    /* (ABI 4) what the row kernels of the job read and write besides the packed CSR entries, for the kernel's OWN byte model
     * (bench.py roofline.frac_own_bytes) and its LDS-atomic floor (one ds_add wave instruction per segment): */
    int64_t cooc_segments;       /* <= 64-entry segments in the job's segment tables (12 B of descriptor each) */
    int64_t cooc_matrix_bytes;   /* bytes of co-rating matrix / panel / block-bound rows the row kernels store */
    int64_t rows_refined;        /* list rows whose score nearly cancels (|score| < c sqrt(n)) and that were scored again in fp64 from the fp32 head rows */
} fy_stats;
int fy_result_stats(fy_result*, fy_stats* out);

/* ------------------------------------------------------------------ NMF / PPC factorisation (produces the H of fy_cluster_assign)
 * Replaces NMFDriver / PPCDriver (M/nmf/AbstractNMFDriver.java:88-150): numberOfIterations rounds of the multiplicative
 * updates, each computing H2 and W2 from the same old (H, W) -- ComputeHJob + HComputationReducer.java:57-75 (or
 * PPCComputeHJob + PPCHComputationReducer.java:61-96) and ComputeWJob + WComputationMapper.java:100-118 -- in fp64 with
 * eps = 1e-12 (MatrixComputationJob.java:41).  Only ratings with score > 0 enter (VectorByItemHDFSMapper.java:37-40).
 * H: number_of_users x k, W: number_of_items x k doubles, row-major, HOST memory, updated in place; row r belongs to id
 * r + 1 (the H / W files are keyed from 1, DataInitialization.createMatrix).  A user (item) in [1, n] without a kept rating
 * fails like the reference's NoSuchElementException ("User %d has not rated any item" / "Item %d has not been rated by
 * anybody"); an id outside the ranges fails too (the reference would hit a null vector). */
typedef struct {
    int32_t number_of_users;           /* "numberOfUsers" */
    int32_t number_of_items;           /* "numberOfItems" */
    int32_t number_of_clusters;        /* "numberOfClusters" = k (<= 256) */
    int32_t number_of_iterations;      /* "numberOfIterations" */
    int32_t ppc;                       /* 0 = NMFDriver, 1 = PPCDriver */
    int32_t normalization_frequency;   /* PPC: the rows of H are L1-normalised when iteration % f == 0 (Java's %, so the
                                          reference's unset key, -1, normalises every iteration); 0 = never */
} fy_nmf_params;
/* stats: nnz / n_users / n_items, ms_prepare (the sorted copies of the ratings), ms_cooc = the iterations alone (H / W resident in
 * HBM), ms_total = everything including the host transfers of H and W in both directions. */
int fy_nmf_factorize(fy_context*, const fy_nmf_params*, const fy_ratings*, double* H_inout, double* W_inout, fy_stats* stats_or_null);

/* ------------------------------------------------------------------ cluster refinement (--usersPerSubCluster / -k2)
 * Replaces RMRecommenderDriver.clusterRefinement / doMappings (M/rmrecommender/RMRecommenderDriver.java:217-266, 298-345):
 * SubClusterMappingJob with its User / ItemMappingReducer, the Mappings mappers and reducers, one PPCDriver run per parent
 * cluster and ClusterAssignmentJob(true) -- for ALL parent clusters in one batched pass on the GPU (csrc/fy_refine.hip).
 *
 * Mappings.  Input: the resident ratings and a parent clustering (map_user / map_cluster, HOST arrays, clusters in
 * [0, number_of_clusters); a later entry of one user replaces the earlier; a member of a cluster outside that range fails with
 * FY_ERR_CLUSTER_RANGE).
 *   users of cluster c : the map's entries (InverseMapper over the `clustering` file): a mapped user without a kept rating is
 *                        still a member;
 *   items of cluster c : the distinct items with score > 0 rated by a user whose getCluster is c
 *                        (ItemByClusterHDFSMapper.java:38-43); a user the map does not name has cluster 0 (Trove's no-entry
 *                        value, AbstractByClusterMapper.java:77-79): its items join cluster 0's items, the user joins no user map;
 *   new ids            : 1 .. n_c (users) and 1 .. m_c (items).  The reference leaves their order to the shuffle; here it is
 *                        ASCENDING RAW ID inside every cluster;
 *   kept ratings       : score > 0, the user has a new id in its cluster and the item one too
 *                        (VectorByItemHDFSMapper.java:48-52, ItemScoreByUserHDFSMapper.java:46-49).
 * Accessors copy to HOST arrays of the caller.  Users / items come cluster after cluster, ascending raw id inside a cluster
 * ("row order": row = position in these arrays).  fy_submap_matrix: the kept ratings as CSR over user rows (by_item = 0: rowptr
 * of n_users + 1, col = item ROW, ascending) or as CSC over item rows (by_item = 1: rowptr of n_items + 1, col = user ROW). */
typedef struct fy_submap fy_submap;
int fy_submap_create(fy_context*, const fy_ratings*, int32_t number_of_clusters, int64_t n_map, const int32_t* map_user,
                     const int32_t* map_cluster, fy_submap** out);
int64_t fy_submap_n_users(const fy_submap*);      /* sum of usersInCluster */
int64_t fy_submap_n_items(const fy_submap*);      /* sum of itemsInCluster */
int64_t fy_submap_nnz(const fy_submap*);          /* kept ratings */
int fy_submap_counts(const fy_submap*, int32_t* users_in_cluster, int32_t* items_in_cluster);   /* number_of_clusters ints each */
int fy_submap_users(fy_submap*, int32_t* raw_user, int32_t* cluster, int32_t* new_id);          /* n_users ints each */
int fy_submap_items(fy_submap*, int32_t* raw_item, int32_t* cluster, int32_t* new_id);          /* n_items ints each */
int fy_submap_matrix(fy_submap*, int by_item, int32_t* rowptr, int32_t* col, float* value);
void fy_submap_destroy(fy_submap*);

/* Refinement.  Parent cluster c gets k_c = ceil(n_c / users_per_sub_cluster) sub-clusters (RMRecommenderDriver.java:239) and
 * its own n_c x k_c H and m_c x k_c W; all parents advance together through number_of_iterations multiplicative updates with
 * the arithmetic of fy_nmf_factorize (fp64, eps 1e-12, H2 and W2 from the old pair, PPC's diagonal terms and L1 normalisation
 * when iteration % normalization_frequency == 0).  Summation orders are fixed: two runs give the same bits.  H and W stay in
 * HBM; what leaves the device is the refined clustering
 *     user    = raw id
 *     cluster = parent * ceil(number_of_users / number_of_clusters) + first index of the row's largest value
 *               (FindSubClusterMapper.java:53, 76; number_of_users is the CONFIGURATION value, not the number of map entries)
 *     count   = users per cluster id, n_counts entries (number_of_clusters x that stride, or more -- see below): long and
 *               sparse in ids, exactly the (map_user, map_cluster, cluster_count) arguments of fy_rm2_prepare with
 *               fy_rm2_params::number_of_clusters = n_counts.
 * REFERENCE QUIRK, reproduced: when some k_c exceeds the stride, ids of neighbouring parents collide (a user of parent c with
 * argmax >= stride lands in the id range of parent c + 1; for the last parent the count array grows beyond K x stride).
 * fy_refine_stats::collisions counts the users with argmax >= stride; nothing is renumbered.
 * Initial matrices: H0 / W0 (HOST, both or neither) hold the per-cluster matrices one after the other in cluster order, rows in
 * new-id order, row-major (sum n_c k_c and sum m_c k_c doubles).  When NULL the device fills them from `seed` (the
 * reference's sub-runs start from unpinned random matrices, AbstractNMFDriver.java:103-109): element (row, col), both from 0,
 * of matrix `which` (0 = H, 1 = W) of parent cluster c is
 *     mix(x) : x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31
 *     z = mix(seed ^ mix(((c << 32) | which) ^ mix((row << 32) | col)))            (64-bit, wrapping: splitmix64's finaliser)
 *     value = ((z >> 11) + 1) * 2^-53                                              in (0, 1]
 * Failures: k_c > 256 (the limit of fy_nmf_factorize) is FY_ERR_UNSUPPORTED and names the parent cluster; a member user
 * without a kept rating fails like the reference's sub-run, "User %d has not rated any item (parent cluster %d)", an item
 * likewise with "Item %d has not been rated by anybody (parent cluster %d)" -- both with the RAW id (only when
 * number_of_iterations > 0; the items of a parent cluster without users are passed over). */
typedef struct {
    int32_t number_of_users;           /* "numberOfUsers": only the id stride ceil(numberOfUsers / numberOfClusters) */
    int32_t number_of_clusters;        /* "numberOfClusters": parent clusters */
    int32_t users_per_sub_cluster;     /* "usersPerSubCluster" (> 0) */
    int32_t number_of_iterations;      /* "numberOfIterations" */
    int32_t ppc;                       /* 0 = NMFDriver, 1 = PPCDriver (what the reference runs) */
    int32_t normalization_frequency;   /* as in fy_nmf_params */
    uint64_t seed;                     /* initial matrices when H0 / W0 are NULL */
} fy_refine_params;
typedef struct {
    double ms_mappings;        /* HIP-event milliseconds: mappings, remapped CSR / CSC, launch tables */
    double ms_iterations;      /* the multiplicative updates alone */
    double ms_assign;          /* argmax, counts and the copy of the clustering to the host */
    double ms_total;
    int64_t launches;          /* kernel and rocPRIM launches of the whole call */
    int64_t sum_users, sum_items, sum_k;   /* sum over the parents of n_c, m_c, k_c */
    int64_t nnz;               /* kept ratings */
    int64_t collisions;        /* users whose argmax >= stride (see above) */
} fy_refine_stats;
typedef struct fy_refined fy_refined;
int fy_cluster_refine(fy_context*, const fy_refine_params*, const fy_ratings*, int64_t n_map, const int32_t* map_user,
                      const int32_t* map_cluster, const double* H0, const double* W0, fy_refined** out);
int64_t fy_refined_n_users(const fy_refined*);
int64_t fy_refined_n_counts(const fy_refined*);
int fy_refined_clustering(const fy_refined*, int32_t* user, int32_t* cluster, int32_t* count);   /* n_users, n_users, n_counts ints */
int fy_refined_layout(const fy_refined*, int32_t* users_in_cluster, int32_t* items_in_cluster, int32_t* sub_clusters);   /* n_c, m_c, k_c */
int64_t fy_refined_h_size(const fy_refined*);     /* sum n_c k_c */
int64_t fy_refined_w_size(const fy_refined*);     /* sum m_c k_c */
int fy_refined_factors(fy_refined*, double* H, double* W);   /* downloads the final factors (tests, diagnostics), layout of H0 / W0 */
int fy_refined_stats(const fy_refined*, fy_refine_stats* out);
void fy_refined_free(fy_refined*);

/* ------------------------------------------------------------------ the Hadoop files on either side of the RM2 job
 * (csrc/fy_seqfile.cpp).  Hadoop 1.2.1 SequenceFile, version 6, uncompressed record format, as the
 * reference's jobs and fixture writers produce it (M/util/DataInitialization.java:155-222, M/rm/RM2HDFSReducer.java:44-50,
 * M/rm/RM2Job.java:110-205).  `path` may be a file, a job output directory (every part file, hidden files skipped) or a
 * MapFile directory.  Readers return malloc'ed arrays: release them with fy_buffer_free.  Host-only: no GPU is touched.
 * PARITY UNPINNED at the byte level (the reference holds no binary fixture); IntPairWritable is Mahout 0.8's, restated as two
 * big-endian int32 -- see the header of csrc/fy_seqfile.cpp. */
int fy_seqfile_read_int_int(const char* path, int64_t* n, int32_t** key, int32_t** value);           /* clustering, clusteringCount */
int fy_seqfile_read_int_double(const char* path, int64_t* n, int32_t** key, double** value);         /* rm2/userSum, rm2/itemColl */
int fy_seqfile_read_intpair_float(const char* path, int64_t* n, int32_t** first, int32_t** second, float** value);   /* ratings, recommendations */
int fy_seqfile_write_int_int(const char* file, int64_t n, const int32_t* key, const int32_t* value);
int fy_seqfile_write_int_double(const char* file, int64_t n, const int32_t* key, const double* value);
int fy_seqfile_write_intpair_float(const char* file, int64_t n, const int32_t* first, const int32_t* second, const float* value);
int fy_mapfile_write_int_double(const char* dir, int64_t n, const int32_t* key, const double* value);   /* rm2/itemColl: data + index */
/* usersFile / itemsFile: a text file with one id per line.  A line that is not an integer (blank, `abc`, `12x`) is skipped like the
 * reference's "itemsFile line ignored" (BaselineAggregateAndRecommendReducer.java:173-179), and so is an id that does not fit
 * int32 (no such id can be in the ratings); blanks around the number and a missing last newline are accepted.  Host-only. */
int fy_idfile_read(const char* path, int64_t* n, int32_t** ids);
void fy_buffer_free(void*);

/* ------------------------------------------------------------------ offline evaluation: hold-out split and ranking metrics
 * (csrc/fy_eval.hip).  The reference ships its item-based recommender as a baseline to compare RM2 against
 * and has no evaluator of its own; these calls say which lists recommend better without moving a list off the GPU.
 *
 * Hold-out split.  Two NEW, independent ratings objects from a resident one; the source is only read and what the jobs kept on it
 * stays valid.  Entry (user, item) goes to *test iff (z >> 40) < floor(fraction * 2^24), all arithmetic modulo 2^64:
 *     k = ((uint64)(uint32) user << 32) | (uint32) item
 *     z = k + seed * 0x9E3779B97F4A7C15
 *     z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 * The decision depends on the key alone: a duplicate key lands on one side, and the side of a rating does not change when other
 * ratings are written (fy_ratings_apply).  Both outputs keep the source order, scores are stored bit for bit, and the id bounds
 * kept with each output are those of its own contents (fy_ratings_apply, rule 5).  fraction outside [0, 1] or NaN is
 * FY_ERR_INVALID_ARGUMENT; 0 gives (a copy, an empty object), 1 the reverse.  On any failure both outputs are NULL. */
int fy_ratings_holdout(fy_context*, const fy_ratings* source, double fraction, uint64_t seed, fy_ratings** train, fy_ratings** test);

/* A list result from rows made elsewhere (for example the reference's own output file read by fy_seqfile_read_intpair_float), so
 * that those lists can be evaluated too: a result of the item-CF list kind (aux = 0, no side outputs, fy_result_stats: recs = n,
 * users_scored = lists).  `location` (FY_HOST / FY_DEVICE) as in fy_ratings_create; the arrays may be freed when the call returns.
 * Rows are taken as given: grouped by user, best first.  A user whose rows form two separate runs is FY_ERR_INVALID_ARGUMENT
 * (checked on the device).  An item named twice in one list is NOT checked and counts twice in every metric.  n > 2^31 - 1 is
 * FY_ERR_UNSUPPORTED. */
int fy_result_create_lists(fy_context*, int64_t n, const int32_t* user, const int32_t* item, const float* value, int location,
                           fy_result** out);

/* The evaluator: prepared once from the test ratings, it computes the ranking metrics of any list result (fy_rm2_score,
 * fy_rm2_score_users, fy_itemcf_recommend*, fy_result_create_lists) where the result lies in HBM.
 * Parameters: cutoffs strictly ascending, each in [1, FY_EVAL_MAX_CUTOFF], 1 <= n_cutoffs <= FY_EVAL_MAX_CUTOFFS.  A test entry is
 * RELEVANT iff (double) score >= relevance_threshold (NaN: never).  Its gain is 1 (FY_EVAL_GAIN_BINARY), score
 * (FY_EVAL_GAIN_LINEAR) or 2^score - 1 (FY_EVAL_GAIN_EXP2), in fp64; every other item has gain 0.  The two graded gains require
 * relevance_threshold > 0.  Anything else is FY_ERR_INVALID_ARGUMENT; a (user, item) that `test` holds twice is
 * FY_ERR_DUPLICATE_RATING; more than 2^31 - 1 test entries or list rows is FY_ERR_UNSUPPORTED.  The evaluator owns its tables: the
 * test ratings may be destroyed after fy_eval_prepare; the evaluator itself is destroyed before its context.  fy_eval_lists refuses
 * with FY_ERR_INVALID_ARGUMENT a result of the item-similarity or item-pairs kind, a result of another context, and a result whose
 * rows live on the host only (fy_rm2_run, fy_itemsim_run: their context is gone).
 * Definitions (fp64; positions p from 1; the list cut at cutoff N; R_u = the relevant items of the list's user):
 *     a list is EVALUATED iff |R_u| > 0
 *     hits_N = |top_N of the list, in R_u|        precision = hits_N / N  (N, not the list's length)        recall = hits_N / |R_u|
 *     AP_N   = (sum over the hit positions p <= N of hits_p / p) / min(|R_u|, N)
 *     RR_N   = 1 / (first hit position <= N), else 0
 *     DCG_N  = sum over p <= N of gain_p / log2(p + 1)
 *     nDCG_N = DCG_N / IDCG_N,  IDCG_N = the same sum over the user's min(N, |R_u|) largest gains in descending order
 * The value column of the lists is never read: -inf and NaN scores are fine, only the row order counts.
 * fy_eval_sums holds SUMS over the evaluated lists, not means: the ranks of a multi-rank job evaluate their own lists and the host
 * adds the sums in rank order (precision = hits / (N * users_evaluated), the other means = sum / users_evaluated, or / relevant_users
 * to count the users that have relevant test items and no list as zeros).  The sums are bit-identical from run to run: per-list
 * values are reduced in a fixed order.  With FY_EVAL_COVERAGE, distinct_items = the number of different items among the first
 * cutoffs[n_cutoffs - 1] rows of all lists OF THIS RESULT (-1 without the flag); the union over the ranks of a multi-rank job is
 * not formed.  ms = HIP-event time of the call.
 * Per-list outputs, both optional HOST arrays in list order: per_user_id_or_null (`lists` ids) and per_user_or_null
 * (lists x n_cutoffs x 5 doubles: hits, recall, AP, RR, nDCG per cutoff; NaN for a list that is not evaluated).  Size them from
 * fy_result_size (an upper bound of `lists`) or call once with NULLs and read `lists`. */
#define FY_EVAL_MAX_CUTOFFS 8
#define FY_EVAL_MAX_CUTOFF 4096
enum { FY_EVAL_GAIN_BINARY = 0, FY_EVAL_GAIN_LINEAR = 1, FY_EVAL_GAIN_EXP2 = 2 };
#define FY_EVAL_COVERAGE 1u
typedef struct {
    int32_t n_cutoffs;
    int32_t cutoffs[FY_EVAL_MAX_CUTOFFS];
    int32_t gain;                 /* FY_EVAL_GAIN_* */
    uint32_t flags;               /* FY_EVAL_COVERAGE */
    double relevance_threshold;
} fy_eval_params;
typedef struct {
    int64_t lists;                    /* lists of the result */
    int64_t users_evaluated;          /* lists whose user has a relevant test entry */
    int64_t lists_without_relevant;   /* lists - users_evaluated */
    int64_t relevant_users;           /* users of `test` with a relevant entry */
    int64_t relevant_entries;
    int64_t distinct_items;           /* FY_EVAL_COVERAGE; -1 otherwise */
    int32_t n_cutoffs;
    int32_t reserved;
    int32_t cutoffs[FY_EVAL_MAX_CUTOFFS];
    int64_t hits[FY_EVAL_MAX_CUTOFFS];        /* per cutoff: sum of hits_N */
    int64_t users_hit[FY_EVAL_MAX_CUTOFFS];   /* evaluated lists with hits_N > 0 */
    double recall[FY_EVAL_MAX_CUTOFFS], ap[FY_EVAL_MAX_CUTOFFS], rr[FY_EVAL_MAX_CUTOFFS], ndcg[FY_EVAL_MAX_CUTOFFS];
    double ms;
} fy_eval_sums;
typedef struct fy_eval fy_eval;
int fy_eval_prepare(fy_context*, const fy_eval_params*, const fy_ratings* test, fy_eval** out);
int fy_eval_lists(fy_eval*, fy_result* lists, fy_eval_sums* out, int32_t* per_user_id_or_null, double* per_user_or_null);
void fy_eval_destroy(fy_eval*);

/* ------------------------------------------------------------------ item-based CF: estimated preferences for named pairs; MAE / RMSE
 * (csrc/fy_itemcf_estimate.hip, csrc/fy_eval.hip).  Mahout's ItemBasedRecommender.estimatePreference asked of
 * the DISTRIBUTED job: estimate(u, i) is the cell (u, i) of the pass fy_itemcf_recommend_prepared runs for the same prepared job, the
 * same max_prefs_per_user and boolean_data, without an allow-list, before the top-N.  It is NOT Mahout's non-distributed
 * estimatePreference (every preference, untruncated similarities).  Restated from the published algorithm like every Mahout class of
 * this package: PARITY UNPINNED.
 * The contributing preferences are the user's kept ones: p >= the max_prefs_per_user-th largest value, ties at the cut kept.  A
 * kept preference j contributes to (u, i) iff row j of the job (its max_similarities_per_item best entries) holds i.  The additions
 * run in the order of the user's preferences, in fp64: num += pref * sim (pref = 1 with boolean_data), den += |sim|, cnt += 1; the
 * finish is the list pass's: (float)(num / den) where cnt > 1, (float) num where cnt > 0 with boolean_data, nothing where num == 0.
 * So wherever a list of fy_itemcf_recommend_prepared holds (u, i), the estimate is that float BIT FOR BIT, and a pair the list pass
 * can never emit has a status that says why.  A kept preference whose row is empty adds nothing, not even its self entry (as in the
 * list pass): its own cell is an ordinary cell.
 * Every asked pair gets exactly one row, in the order asked; a pair asked twice is answered twice.  Row: key0 = user, key1 = item
 * (as asked), value = the estimate (NaN unless the status is FY_ESTIMATE_OK), aux = the status, the FIRST of these that applies: */
enum {
    FY_ESTIMATE_OK = 0,               /* value is the prediction */
    FY_ESTIMATE_UNKNOWN_USER = 1,     /* no kept preference: an id outside the data, or a negative id */
    FY_ESTIMATE_UNKNOWN_ITEM = 2,     /* nobody rated it: the item has no column */
    FY_ESTIMATE_OWN_PREFERENCE = 3,   /* the item is one of the user's kept (strongest) preferences: the (j, NaN) self entry of the list
                                         pass.  An item the user rated below the cut is an ordinary cell, as in the list pass */
    FY_ESTIMATE_TOO_FEW = 4,          /* fewer than two contributing preferences (fewer than one with boolean_data) */
    FY_ESTIMATE_ZERO_NUMERATOR = 5,   /* numerator exactly 0: the reducer's nonZeroes() skip */
    FY_ESTIMATE_NOT_A_NUMBER = 6      /* the arithmetic gave NaN (a NaN preference or similarity): the list pass drops such a cell */
};
/* Pairs: two arrays of raw ids, FY_HOST or FY_DEVICE (HBM of the job's context); they may be freed when the call returns.
 * fy_itemcf_estimate_ratings asks for the (user, item) columns of a resident ratings object of the job's context in its COO order
 * (typically the test side of fy_ratings_holdout: no id leaves the GPU); its scores are not read.
 * (rank, world) of fy_itemcf_params cut the PAIR LIST into contiguous ranges [n rank / world, n (rank + 1) / world): a rank's result
 * holds its own range and remembers the offset of its first pair (fy_itemcf_estimate_stats.pair_offset; fy_eval_estimates reads
 * it).  num_recommendations is ignored.  The failures are fy_itemcf_recommend_prepared's: a job prepared with world != 1 or with
 * min_prefs_per_user / max_prefs_per_user is FY_ERR_UNSUPPORTED, NULL arguments and max_prefs_per_user <= 0 are
 * FY_ERR_INVALID_ARGUMENT, more than 2^31 - 1 pairs are FY_ERR_UNSUPPORTED.  Zero pairs, or a job over an empty preference
 * matrix (every pair: FY_ESTIMATE_UNKNOWN_USER), build nothing.
 * The rows the estimates need are the rows of the kept preferences of the asked users; they come from and stay in the job's row
 * store, shared with fy_itemcf_recommend_prepared in both directions.
 * Work: equal pairs form one target; a user's distinct targets are cut into chunks of FY_ICF_EST_CHUNK (default 256) and ONE WAVE
 * per (user, chunk) walks the user's rows once, so row_entries_walked is paid per chunk, not per pair.  Nothing is sized by the
 * catalogue: no dense accumulator row, no top-N, no global atomics on the cells.
 * fy_result_stats: nnz, n_users, n_items (the job's), recs = rows, users_scored = distinct users with at least one OK pair,
 * pair_contribs, cooc_launches (= batches), score_launches, ms_tables (keys, sort, thresholds, the set J), ms_cooc (row kernel,
 * merge, store fill), ms_score (the estimate kernel), ms_total; ms_prepare = 0 and ms_topn = 0.
 * The result is a kind of its own: fy_eval_lists, fy_itemsim_pairs and fy_itemcf_recommend* refuse it with
 * FY_ERR_INVALID_ARGUMENT; fy_result_key0 / key1 / value / aux read it. */
typedef struct {
    int64_t n_pairs;
    const int32_t* users;     /* raw user ids */
    const int32_t* items;     /* raw item ids */
    int location;             /* FY_HOST | FY_DEVICE */
} fy_itemcf_pairs;
typedef struct {
    int64_t pairs_asked;         /* rows of this result (this rank's range of the pair list) */
    int64_t pair_offset;         /* position of the first of them in the whole pair list */
    int64_t by_status[8];        /* rows per FY_ESTIMATE_* code */
    int64_t users_known;         /* distinct users of the range with a kept preference */
    int64_t targets;             /* distinct (known user, known item) pairs: what the estimate kernel computes */
    int64_t chunks;              /* (user, chunk of targets) = waves of the estimate kernel */
    int64_t items_needed;        /* these six as in fy_itemcf_request_stats */
    int64_t rows_built;
    int64_t rows_from_store;
    int64_t rows_stored;
    int64_t pair_contribs;
    int64_t batches;
    int64_t row_entries_walked;  /* sum over the chunks of sum over the user's kept preferences j of the entries of row j */
} fy_itemcf_estimate_stats;
int fy_itemcf_estimate_prepared(fy_itemsim_job*, const fy_itemcf_params*, const fy_itemcf_pairs*, fy_result** out);
int fy_itemcf_estimate_ratings(fy_itemsim_job*, const fy_itemcf_params*, const fy_ratings* asked, fy_result** out);
int fy_result_itemcf_estimate_stats(fy_result*, fy_itemcf_estimate_stats* out);   /* FY_ERR_STATE on any other result */

/* Rating-error sums of an estimates result against the true scores (Mahout's AverageAbsoluteDifferenceRecommenderEvaluator and
 * RMSRecommenderEvaluator).  Row r of `estimates` is compared with entry pair_offset + r of `truth` (a resident ratings object of the
 * same context, in its COO order): the (user, item) of the two must agree row for row, which is checked on the device; a
 * disagreement, or a range that does not fit into `truth`, is FY_ERR_INVALID_ARGUMENT.  Only FY_ESTIMATE_OK rows whose truth score is
 * finite enter the sums: e = (double) estimate - (double) truth score, the estimate first clamped into [clamp_lo, clamp_hi] when
 * has_clamp (clamp_lo > clamp_hi or a NaN bound: FY_ERR_INVALID_ARGUMENT; params == NULL: no clamp).
 * SUMS, not means: MAE = sum_abs / estimated, RMSE = sqrt(sum_sq / estimated), bias = sum_err / estimated, coverage = estimated /
 * pairs; the ranks of a multi-rank job add their sums in rank order like fy_eval_sums.  The three sums are bit-identical from run to
 * run: per-thread partial sums over fixed slices in a fixed order, no floating-point atomics. */
typedef struct {
    int32_t has_clamp;
    int32_t reserved;
    double clamp_lo, clamp_hi;
} fy_eval_error_params;
typedef struct {
    int64_t pairs;                /* rows of `estimates` */
    int64_t estimated;            /* rows that entered the sums */
    int64_t truth_not_finite;     /* FY_ESTIMATE_OK rows left out because the truth score is NaN or infinite */
    int64_t by_status[8];         /* rows per FY_ESTIMATE_* code */
    double sum_abs, sum_sq, sum_err;
    double ms;                    /* HIP-event time of the call */
} fy_eval_errors;
int fy_eval_estimates(fy_context*, fy_result* estimates, const fy_ratings* truth, const fy_eval_error_params* params_or_null,
                      fy_eval_errors* out);

/* ------------------------------------------------------------------ item-based CF: named pairs explained by their contributing
 * preferences (csrc/fy_itemcf_because.hip).  Mahout's ItemBasedRecommender.recommendedBecause(user, item,
 * howMany) asked of the DISTRIBUTED job: the "because you liked ..." line under a recommendation.  The explanation of a pair (u, i)
 * is the decomposition of the cell (u, i) of the list pass, the very cell fy_itemcf_estimate_prepared finishes for the same prepared
 * job, the same max_prefs_per_user and boolean_data.  It is NOT Mahout's non-distributed recommendedBecause, which sees every
 * preference and untruncated similarities; Mahout's source is not at hand, so the ranking is DEFINED here, not restated: PARITY
 * UNPINNED like the rest of the package.
 * Kept preferences of u: as everywhere, p >= the max_prefs_per_user-th largest value, ties at the cut kept.  A kept preference j is a
 * CONTRIBUTOR of (u, i) iff its row in the job's store is non-empty and holds i.  A contributor carries
 *     sim   the float of the store: bit for bit what fy_itemsim_rows returns for (j, i)
 *     pref  the stored float, or 1.0f with boolean_data
 * and its weight is (double) pref * (double) sim, the very term the numerator receives (the product of two floats is exact in fp64,
 * so the order below involves no rounding).  Within a pair the contributors are ordered by descending weight, equal weights by
 * ascending raw id of the contributing item, a NaN weight after every number (also by ascending id).  At most how_many are LISTED
 * per pair, 1 <= how_many <= FY_BECAUSE_MAX.
 * Per pair, whether or not rows are listed: `estimate` and `status` are exactly fy_itemcf_estimate_prepared's value and
 * FY_ESTIMATE_* code for that pair, BIT FOR BIT (the additions run in the order of the user's preferences, __dmul_rn / __dadd_rn in
 * fp64, with the same finish), and `contributors` counts all contributing preferences, listed or not (the estimate's cnt).  A pair
 * with a known user and a known item lists its contributors whatever its status (FY_ESTIMATE_TOO_FEW, _ZERO_NUMERATOR,
 * _NOT_A_NUMBER and _OWN_PREFERENCE pairs still have terms); FY_ESTIMATE_UNKNOWN_USER and _UNKNOWN_ITEM pairs list none.  Every
 * asked pair is answered once, in the order asked; a pair asked twice is answered twice.
 * The result is a kind of its own.  Rows are grouped by asked pair in the order asked: key0 = user, key1 = the contributing item
 * (raw id), value = sim, aux = the index of the pair inside this rank's range.  fy_result_because_view gives host pointers owned by
 * the result (valid until fy_result_free, like fy_result_key0): the rows of pair t are start[t] .. start[t + 1], per pair the ids as
 * asked, estimate, status, contributors, and per row pref.  fy_eval_lists, fy_eval_estimates, fy_itemsim_pairs and
 * fy_itemcf_recommend* refuse the kind with FY_ERR_INVALID_ARGUMENT.
 * Arguments: the pairs as for fy_itemcf_estimate_prepared; (rank, world) of fy_itemcf_params cut the pair list into the same
 * contiguous ranges; num_recommendations is ignored.  The failures are fy_itemcf_estimate_prepared's (a job prepared with world != 1
 * or with min_prefs_per_user / max_prefs_per_user: FY_ERR_UNSUPPORTED; NULL arguments, max_prefs_per_user <= 0:
 * FY_ERR_INVALID_ARGUMENT; more than 2^31 - 1 pairs, or pairs x how_many beyond 2^31 - 1: FY_ERR_UNSUPPORTED) plus how_many outside
 * [1, FY_BECAUSE_MAX]: FY_ERR_INVALID_ARGUMENT.  Zero pairs, or a job over no preferences, build nothing.  The rows the call needs
 * come from and stay in the job's row store, shared in both directions with fy_itemcf_recommend_prepared and the estimates; the
 * store changes no bit of the answer.
 * Work: equal pairs form one target and ONE WAVE per distinct target walks the user's kept rows, so row_entries_walked is paid per
 * target.  Nothing is sized by the catalogue.
 * fy_result_stats follows the estimates: recs = rows, users_scored = distinct users with at least one OK pair, ms_tables / ms_cooc /
 * ms_score (the explanation kernel and the compaction) / ms_total; ms_prepare = ms_topn = 0. */
#define FY_BECAUSE_MAX 64
typedef struct {
    int64_t n_pairs;
    const int64_t* start;          /* n_pairs + 1: rows of pair t = start[t] .. start[t + 1] */
    const int32_t* user;           /* per pair, as asked */
    const int32_t* item;
    const float* estimate;         /* per pair: NaN unless status is FY_ESTIMATE_OK */
    const int32_t* status;         /* per pair: FY_ESTIMATE_* */
    const int32_t* contributors;   /* per pair: all contributing preferences, listed or not */
    const float* pref;             /* per row */
} fy_itemcf_because_view;
typedef struct {
    int64_t pairs_asked;         /* pairs of this result (this rank's range of the pair list) */
    int64_t pair_offset;         /* position of the first of them in the whole pair list */
    int64_t by_status[8];        /* pairs per FY_ESTIMATE_* code */
    int64_t users_known;         /* distinct users of the range with a kept preference */
    int64_t targets;             /* distinct (known user, known item) pairs = waves of the explanation kernel */
    int64_t rows;                /* rows listed */
    int64_t contributors;        /* sum of `contributors` over the asked pairs */
    int64_t items_needed;        /* these six as in fy_itemcf_estimate_stats */
    int64_t rows_built;
    int64_t rows_from_store;
    int64_t rows_stored;
    int64_t pair_contribs;
    int64_t batches;
    int64_t row_entries_walked;  /* sum over the distinct targets of the entries of the rows of the user's kept preferences */
} fy_itemcf_because_stats;
int fy_itemcf_because_prepared(fy_itemsim_job*, const fy_itemcf_params*, const fy_itemcf_pairs*, int32_t how_many, fy_result** out);
int fy_result_because_view(fy_result*, fy_itemcf_because_view* out);             /* FY_ERR_STATE on any other result */
int fy_result_itemcf_because_stats(fy_result*, fy_itemcf_because_stats* out);   /* FY_ERR_STATE on any other result */

/* ------------------------------------------------------------------ item-based CF: lists for given profiles and pending writes
 * fy_itemcf_recommend_profiles (csrc/fy_itemcf_profiles.hip) runs the list pass of
 * fy_itemcf_recommend_prepared over preference vectors the CALLER hands in instead of rows of the ratings the job was prepared on:
 * an anonymous or brand-new user's whole profile (Mahout's PlusAnonymousUserDataModel), or a resident user's row with pending
 * writes applied ("what if I rated this", or a write the job has not been prepared on yet).  The similarity rows stay as prepared:
 * nothing of the job -- similarities, norms, popularity ranks, its own CSR -- follows the writes.  The job and its warm row store
 * serve the call as they stand; no re-prepare.
 * The profiles are HOST arrays in CSR form: profile p holds the entries start[p] .. start[p + 1] of item / score / remove.
 * Composition, per profile:
 *   1. The entries are applied in the order given and the LAST entry per item counts, whether it is a write or a delete
 *      (remove[e] != 0; its score is ignored): fy_ratings_apply's rule 1.
 *   2. An entry whose item has no column -- nobody rated it in the prepared ratings, or its id is negative -- is dropped and counted
 *      (entries_unknown_item) before rule 1 sees it: such an item has no similarity row and can be neither a preference nor a
 *      recommendation of this job.
 *   3. FY_PROFILE_ON_RESIDENT: the entries are applied on top of the job's own row of `user[p]`, i.e. EVERY preference of that row
 *      (before any max_prefs_per_user cut); an entry for an item of the row replaces or deletes it.  A user the job does not know
 *      starts empty and is counted (users_unknown).  FY_PROFILE_WHOLE: the starting row is empty, whoever `user[p]` is.
 *   4. Scores are taken as given, bit for bit, AS THE JOB'S RATINGS HOLD THEM: a job prepared on shifted ratings (fy_ratings_shifted)
 *      wants shifted scores, and the shift is the caller's to apply.  A score <= 0 is a stored preference, not a delete.
 *   5. The composed profile is ordered as a resident row is: ascending popularity-rank column.
 * Then the list pass, unchanged: the max_prefs_per_user threshold on the COMPOSED profile with ties at the cut kept, the set J of the
 * kept preferences, the missing similarity rows built and kept in the job's row store (shared in both directions with
 * fy_itemcf_recommend_prepared, the estimates and the explanations), accumulate in preference order, finalize ((j, NaN) self entry,
 * numerator == 0 skip, at least two contributing preferences -- one with boolean_data --, the allow-list), top-N.  A composed profile
 * that equals a resident row therefore gets that user's list of fy_itemcf_recommend_prepared BIT FOR BIT.
 * Result: the ordinary list kind (fy_eval_lists takes it).  Rows are grouped by profile IN THE ORDER GIVEN, best first; the user
 * column holds user[p], a label that may repeat (two what-if variants of one user give two groups).  A profile that composes to
 * nothing, or whose cells hold no prediction, gets no rows.  (rank, world) of fy_itemcf_params cut the PROFILE LIST into contiguous
 * ranges [n rank / world, n (rank + 1) / world).  items_only: NULL, or a filter with has_items (the allow-list) and has_users == 0.
 * Failures: everything fy_itemcf_recommend_prepared refuses (numRecommendations, maxPrefsPerUser, rank / world; a job prepared with
 * world != 1 or with min / max_prefs_per_user: FY_ERR_UNSUPPORTED) with the same code; NULL user / start with n_profiles > 0, NULL
 * item / score with entries, start[0] != 0 or start decreasing, base outside the enum, n_profiles < 0, has_users set in the filter:
 * FY_ERR_INVALID_ARGUMENT; more than 2^31 - 1 profiles or entries, or more than 2^31 - 1 preferences to compose (this rank's entries
 * plus the resident rows they are applied on): FY_ERR_UNSUPPORTED.  All of these are found on the host before any launch.  Zero
 * profiles, or a job over no preferences, builds nothing and returns an empty result.  A failed call leaves the job and its row
 * store usable.
 * Work: sized by the request -- this rank's entries plus the resident rows of the users they name (one stable radix sort of that many
 * 64-bit keys, a scan, a scatter) -- then exactly what fy_itemcf_recommend_prepared pays for as many users.
 * fy_result_stats as for fy_itemcf_recommend_prepared (users_scored = profiles that received a list; ms_tables includes the ingest).
 * Counters (all but profiles_asked over this rank's range of profiles):
 *   profiles_asked        n_profiles
 *   profiles_mine         profiles of this rank's range
 *   profiles_scored       profiles that received a list
 *   profiles_empty        profiles whose composed preference vector is empty
 *   users_unknown         FY_PROFILE_ON_RESIDENT: profiles whose user the job does not know (0 with FY_PROFILE_WHOLE)
 *   entries               entries of the profiles
 *   entries_unknown_item  entries dropped by rule 2
 *   entries_superseded    entries with a column that are not the last of their (profile, item)
 *   removes_hit           last entries that are deletes of an item of the resident row
 *   removes_missed        last entries that are deletes of an item the starting row does not hold (every one with FY_PROFILE_WHOLE)
 *   prefs_composed        preferences of all composed profiles
 *   items_needed .. batches   the six row-store fields of fy_itemcf_request_stats */
enum { FY_PROFILE_WHOLE = 0, FY_PROFILE_ON_RESIDENT = 1 };
typedef struct {
    int64_t n_profiles;
    const int32_t* user;     /* n_profiles: the label written to the result's user column; with ON_RESIDENT also the resident user id */
    const int64_t* start;    /* n_profiles + 1 offsets into item / score / remove, non-decreasing from 0 */
    const int32_t* item;     /* raw item ids */
    const float*   score;    /* preferences as the job's ratings hold them (a ratingShift is the caller's to apply) */
    const uint8_t* remove;   /* NULL: no deletes; else non-zero = delete this item from the profile */
    int32_t base;            /* FY_PROFILE_WHOLE / FY_PROFILE_ON_RESIDENT */
} fy_itemcf_profiles;        /* host arrays; they may be freed when the call returns */
typedef struct {
    int64_t profiles_asked, profiles_mine, profiles_scored, profiles_empty, users_unknown;
    int64_t entries, entries_unknown_item, entries_superseded, removes_hit, removes_missed, prefs_composed;
    int64_t items_needed, rows_built, rows_from_store, rows_stored, pair_contribs, batches;
} fy_itemcf_profile_stats;
int fy_itemcf_recommend_profiles(fy_itemsim_job*, const fy_itemcf_params*, const fy_itemcf_profiles*,
                                 const fy_itemcf_filter* items_only /* may be NULL; has_users must be 0 */, fy_result** out);
int fy_result_itemcf_profile_stats(fy_result*, fy_itemcf_profile_stats* out);   /* FY_ERR_STATE on any other result */

/* ------------------------------------------------------------------ RM2 on request: lists for given profiles and pending writes
 * fy_rm2_score_profiles (csrc/fy_rm2_profiles.hip) scores item sets the CALLER hands in on a prepared RM2 job
 * whose global statistics are in place (as fy_rm2_score_users): an anonymous or brand-new visitor's whole profile, or a resident
 * user's row with pending writes applied.  Nothing of the job follows the writes: s_v, p(i|C), b, G, the clustering and U_c stay as
 * prepared.  The call may be made any number of times, before or after fy_rm2_score / fy_rm2_score_users, and leaves the job as it
 * was.  A user's own rating VALUES never enter that user's scores, only the SET of rated items does, so a pending write changes
 * which rows G[j][.] are summed, which columns are masked, and the user's own subtracted term.
 * The profiles are HOST arrays in CSR form, exactly like fy_itemcf_profiles (user = label, start, item, score, remove, base), plus
 *   cluster      n_profiles: the cluster a FY_PROFILE_WHOLE profile is scored in; ignored with FY_PROFILE_ON_RESIDENT (may be NULL)
 *   rank, world  cut the PROFILE LIST into contiguous ranges [n rank / world, n (rank + 1) / world)
 * Composition, per profile:
 *   1. The entries are applied in the order given and the LAST entry per item counts, whether it is a write or a delete
 *      (remove[e] != 0; its score is ignored).
 *   2. An entry whose item has no column in the profile's cluster -- nobody of that cluster rated it in the prepared ratings, the
 *      job does not know the id, or the id is negative -- is dropped and counted (entries_unknown_item) before rule 1 sees it.
 *   3. A last entry whose score is not > 0 (zero, negative, NaN) is not a kept rating: the `score > 0` filter of the prep.  It
 *      removes the item, like a delete, and is counted (entries_nonpositive).
 *   4. FY_PROFILE_ON_RESIDENT: the entries go on top of the job's own row of user[p], and the cluster is that user's.  A user the
 *      job does not know, or one that is not in this job's share, gets no list (users_unknown); a user with id < filterUsers gets
 *      no list (users_filtered).  The entries of such a profile are counted in `entries` and not looked at any further.
 *   5. FY_PROFILE_WHOLE: the starting row is empty, the cluster is cluster[p], filterUsers is not applied.
 *   6. The composed profile is ordered as a resident row is: ascending cluster-local column (rank order).
 * An empty composed profile gets no list (profiles_empty); so does a profile with no candidate left (n' >= I_c).
 * Scoring (Jelinek-Mercer), for every candidate i of I_c outside the profile, n' = |profile|:
 *   ON_RESIDENT  score = (n' - 1) ln M - n' ln U_c + sum_{j in profile} ln sum_{v in c, v != u} c_vi c_vj; with x_u. the PREPARED
 *                row of u (0 where it holds nothing) the inner sum is (1-l)^2 (G[j][i] - x_uj x_ui) + q_j (b_i - x_ui) + a_i e_uj,
 *                e_uj = (1-l)(b_j - x_uj) + l (U_c - 1) p_j, q_j = l (1-l) p_j, a_i = l p_i, every difference clamped at 0.  Where u
 *                is the ONLY rater of i or of j in the cluster, G - x_uj x_ui and the matching b - x are exactly 0 (ln 0 = -inf at
 *                lambda = 0, as the full job gives).
 *   WHOLE        the profile is the (U_c + 1)-th member of its cluster: all U_c residents are neighbours, there is no own term:
 *                (n' - 1) ln M - n' ln(U_c + 1) + sum_j ln[(1-l)^2 G[j][i] + q_j b_i + a_i ((1-l) b_j + l U_c p_j)].
 * List length min(numberOfRecommendations, I_c - n'), the (float) cast, ties by ascending item id; the top-N kernels and the list
 * length limit of fy_rm2_score_users apply.
 * Result: the ordinary list kind (fy_eval_lists takes it).  Rows are grouped by profile IN THE ORDER GIVEN, best first; the user
 * column holds the label, which may repeat; the cluster column holds the cluster scored in.
 * Bit-level promises: an ON_RESIDENT profile whose composed item set equals the resident row gets that user's rows of
 * fy_rm2_score_users BIT FOR BIT; a profile's rows do not depend on the other profiles of the call, their order, workspace_bytes,
 * FY_REQ_CHUNK or (rank, world).
 * Failures, leaving the job usable.  FY_ERR_INVALID_ARGUMENT: NULL user / start with profiles, NULL item / score with entries,
 * start[0] != 0 or start decreasing, base outside the enum, n_profiles < 0, rank / world out of range, WHOLE with cluster == NULL
 * or a cluster[p] outside [0, numberOfClusters) or naming an empty cluster.  FY_ERR_UNSUPPORTED: a job with FY_RM2_ESTIMATOR_RM1; a
 * job with Dirichlet-prior or absolute-discounting smoothing (deliberately out of scope: the own-term algebra above is the
 * Jelinek-Mercer one); a job with collectives installed or prepared with world != 1; more than 2^31 - 1 profiles, entries or
 * elements to compose.  These are found on the host before any launch.  FY_ERR_OUT_OF_MEMORY: one profile whose own slab rows
 * exceed workspace_bytes (found when the batches are planned, before any slab is built; the message names the profile's position
 * and label).  Zero profiles, or a job over no ratings, gives an empty result.
 * fy_result_stats as for fy_rm2_score_users (users_scored = profiles_scored; ms_tables includes the ingest).  Counters (all but
 * profiles_asked over this rank's range):
 *   profiles_asked / _mine / _scored / _empty   asked; of this rank's range; that received a list; that composed to nothing
 *   users_unknown, users_filtered               rule 4
 *   entries                                     entries of the profiles
 *   entries_unknown_item, entries_nonpositive   rules 2 and 3
 *   entries_superseded                          entries with a column that are not the last of their (profile, item)
 *   removes_hit / removes_missed                last entries that are deletes of an item the resident row holds / does not hold
 *   items_composed                              items of all composed profiles
 *   clusters_touched .. slab_pair_contribs      as in fy_rm2_request_stats, over the profiles that received a list */
typedef struct {
    int64_t n_profiles;
    const int32_t* user;     /* n_profiles: the label of the result's user column; with ON_RESIDENT also the resident user id */
    const int64_t* start;    /* n_profiles + 1 offsets into item / score / remove, non-decreasing from 0 */
    const int32_t* item;     /* raw item ids */
    const float*   score;    /* only score > 0 matters: the values never enter the scores */
    const uint8_t* remove;   /* NULL: no deletes; else non-zero = delete this item from the profile */
    const int32_t* cluster;  /* n_profiles with FY_PROFILE_WHOLE; ignored (may be NULL) with FY_PROFILE_ON_RESIDENT */
    int32_t base;            /* FY_PROFILE_WHOLE / FY_PROFILE_ON_RESIDENT */
    int32_t rank, world;     /* the range of the profile list this call serves; 0, 1 = all of it */
} fy_rm2_profiles;           /* host arrays; they may be freed when the call returns */
typedef struct {
    int64_t profiles_asked, profiles_mine, profiles_scored, profiles_empty, users_unknown, users_filtered;
    int64_t entries, entries_unknown_item, entries_nonpositive, entries_superseded, removes_hit, removes_missed, items_composed;
    int64_t clusters_touched, batches, slab_rows, slab_bytes_peak, slab_pair_contribs;
} fy_rm2_profile_stats;
int fy_rm2_score_profiles(fy_rm2_job*, const fy_rm2_profiles*, fy_result** out);
int fy_result_rm2_profile_stats(fy_result*, fy_rm2_profile_stats* out);   /* FY_ERR_STATE on any other result */

/* ------------------------------------------------------------------ fold-in: assign given profiles to clusters from the standing factors
 * (csrc/fy_foldin.hip).  fy_rm2_score_profiles scores a FY_PROFILE_WHOLE profile "as one more member of the
 * cluster named in `cluster`"; this is the call that produces that cluster without a new factorisation and without a prepare.  The
 * item factors W of the last PPC / NMF run are held FIXED, the reference's own H update (HComputationReducer.java:57-75 /
 * PPCHComputationReducer.java:61-96) runs for the given rows alone, and the cluster is the argmax (FindClusterMapper.java:37-45; with a
 * refined level FindSubClusterMapper.java:46-76 on the parent's factors).  All of it in fp64 with eps = 1e-12, as fy_nmf_factorize.
 *
 * Model.  fy_foldin_create puts W (number_of_items x k doubles, row r = item id r + 1; FY_HOST or FY_DEVICE) into HBM and forms
 * C = W^T W exactly as the H half of fy_nmf_factorize forms it (same kernels, same summation order: the same bits).  The model is
 * created once and serves any number of fy_foldin_assign calls.  count_or_null (HOST, n_count ints: a `clusteringCount`) builds a mask of
 * ALLOWED columns: column j may win the argmax only when j < n_count and count[j] > 0 -- fy_rm2_score_profiles refuses an empty
 * cluster.  The mask touches the argmax alone, never the iterations.  NULL: every column is allowed.
 * fy_foldin_add_level adds the refined level of fy_cluster_refine (once): one block per parent cluster c = top-level column c, n_parents
 * = k.  HOST arrays in the layout of fy_submap_counts / fy_submap_items / fy_refined_layout / fy_refined_factors: items_in_cluster
 * (m_c), sub_clusters (k_c <= 256; 0 for a parent without users), item_raw (the parents' item lists one after the other, raw ids
 * ASCENDING inside a parent; row = position), W_ragged (the m_c x k_c matrices one after the other), stride = ceil(numberOfUsers /
 * numberOfClusters).  count_or_null (the refined, long `clusteringCount`): sub-cluster j of parent c is allowed when c * stride + j <
 * n_count and count[c * stride + j] > 0, and top-level column c is allowed when any of its k_c sub-clusters is (this REPLACES the mask
 * of fy_foldin_create); NULL: the sub-clusters are unmasked and the top-level mask stays as it is.
 *
 * Profiles: the HOST CSR of fy_itemcf_profiles (user = label, start, item, score, remove).  Only WHOLE profiles are taken (base must be
 * FY_PROFILE_WHOLE): a resident user's row with pending writes is composed by the caller (Ratings.to_host / fy_ratings_copy_out plus the
 * writes).  Composition, per profile, counted like the other profile calls:
 *   1. an entry whose item id is outside [1, number_of_items] is dropped and counted (entries_out_of_range) before rule 2 sees it;
 *   2. the entries are applied in the order given and the LAST entry per item counts (entries_superseded: the others);
 *   3. a last entry that is a delete (remove[e] != 0) removes the item (entries_removed);
 *   4. a last entry whose score is not > 0 (zero, negative, NaN) removes the item (entries_nonpositive): the factorisation's
 *      kept-rating rule;
 *   5. the composed profile is in ascending item id, the order of the factorisation's rows.
 * Assignment, per profile with composed entries (item_i, a_i):
 *   x      = sum_i a_i W[item_i - 1][:]   in entry order: chunks of 512 entries each summed from 0.0, the chunk sums added from 0.0
 *            (the order fy_nmf_factorize sums a user's row in);
 *   h      = h0[p][:] (h0: HOST, n_profiles x k, rows of ALL profiles of the list; top level only) or uniform 1 / k;
 *   `iterations` times:  y = C h;  NMF: h_c <- h_c x_c / (y_c + eps);  PPC: d = h.y, e = h.x, h_c <- h_c clamp(x_c + d) /
 *            (clamp(y_c + e) + eps) (clamp: +-infinity -> +-DBL_MAX), then h <- h / |h|_1 when normalization_frequency != 0 and
 *            it % normalization_frequency == 0 (C remainder; -1 normalises always), it = first_iteration, first_iteration + 1, ...;
 *   parent = first index of the strictly largest ALLOWED value of h (NaN never wins).
 * h0 = the row's H, first_iteration = 1 and one iteration give the row fy_nmf_factorize would give it in its first iteration from the
 * same W, BIT FOR BIT.  With a refined level every profile then runs on the block of its parent c, over its entries whose item has a
 * row in parent c (same summation order over those entries), from uniform 1 / k_c, and cluster = c * stride + argmax; an argmax >=
 * stride is kept and counted (collisions): the reference's quirk, as fy_cluster_refine documents it.  Without one cluster = parent.
 * Status per profile: FY_FOLDIN_OK; FY_FOLDIN_EMPTY (composed to nothing); FY_FOLDIN_NO_CLUSTER (no allowed column holds a value >
 * -infinity, at either level); FY_FOLDIN_EMPTY_IN_PARENT (none of its items has a row in the parent: `parent` is still reported).
 * cluster = -1 unless the status is OK; parent = -1 with EMPTY and NO_CLUSTER.  The factor rows are kept whatever the status: top
 * level n x k; second level ragged, offset[p] .. offset[p + 1] = the k_c values of profile p (none where level 2 did not run).
 * (rank, world) cut the PROFILE LIST into contiguous ranges [n rank / world, n (rank + 1) / world); the result holds this rank's
 * profiles in the order given.  A profile's outputs do not depend on the other profiles, their order, or the cut.
 * Failures, all found on the host before any launch, leaving the model usable.  FY_ERR_INVALID_ARGUMENT: NULL context / params / W /
 * out, number_of_items or number_of_clusters <= 0, location outside the enum, count NULL with n_count > 0 or n_count < 0;
 * fy_foldin_add_level: n_parents != k, NULL arrays, negative m_c / k_c, stride <= 0, an item list that is not strictly ascending;
 * fy_foldin_assign: NULL model / profiles / out, base other than FY_PROFILE_WHOLE, n_profiles < 0, NULL user / start with profiles,
 * NULL item / score with entries, start[0] != 0 or start decreasing, iterations or first_iteration < 0, rank / world out of range.
 * FY_ERR_UNSUPPORTED: number_of_clusters or a k_c above 256 (the factorisation's limit), more than 2^31 - 1 profiles or entries, a
 * refined cluster id beyond 2^31 - 1.  FY_ERR_STATE: a second fy_foldin_add_level.
 * Counters (all but profiles_asked over this rank's range): profiles_asked / _mine; entries and the four rules' counters;
 * items_composed; profiles_assigned / _empty / _no_cluster / _empty_in_parent (the four statuses); items_in_parent (entries that
 * entered a level-2 sum); collisions; launches (kernel and rocPRIM launches); HIP-event milliseconds per phase. */
enum { FY_FOLDIN_OK = 0, FY_FOLDIN_EMPTY = 1, FY_FOLDIN_NO_CLUSTER = 2, FY_FOLDIN_EMPTY_IN_PARENT = 3 };
typedef struct {
    int32_t number_of_items;           /* "numberOfItems": rows of W */
    int32_t number_of_clusters;        /* "numberOfClusters" = k (<= 256) */
    int32_t ppc;                       /* 0 = NMFDriver's H update, 1 = PPCDriver's */
    int32_t normalization_frequency;   /* as in fy_nmf_params */
} fy_foldin_params;
typedef struct {
    int64_t profiles_asked, profiles_mine, profiles_assigned, profiles_empty, profiles_no_cluster, profiles_empty_in_parent;
    int64_t entries, entries_out_of_range, entries_superseded, entries_removed, entries_nonpositive, items_composed;
    int64_t items_in_parent, collisions, launches;
    double ms_ingest, ms_level1, ms_level2, ms_total;
} fy_foldin_stats;
typedef struct fy_foldin fy_foldin;
typedef struct fy_foldin_result fy_foldin_result;
int fy_foldin_create(fy_context*, const fy_foldin_params*, const double* W, int location, const int32_t* count_or_null, int64_t n_count,
                     fy_foldin** out);
int fy_foldin_add_level(fy_foldin*, int32_t n_parents, const int32_t* items_in_cluster, const int32_t* sub_clusters, const int32_t* item_raw,
                        const double* W_ragged, int32_t stride, const int32_t* count_or_null, int64_t n_count);
int fy_foldin_assign(fy_foldin*, const fy_itemcf_profiles* profiles, int32_t iterations, int32_t first_iteration, const double* h0_or_null,
                     int32_t rank, int32_t world, fy_foldin_result** out);
int64_t fy_foldin_result_n(const fy_foldin_result*);                                /* this rank's profiles */
int fy_foldin_result_assignment(const fy_foldin_result*, int32_t* label, int32_t* cluster, int32_t* parent, int32_t* status);   /* n ints each */
int fy_foldin_result_factors(fy_foldin_result*, double* H);                         /* n x k doubles: the top-level rows */
int64_t fy_foldin_result_sub_size(const fy_foldin_result*);                         /* doubles of all second-level rows */
int fy_foldin_result_sub_factors(fy_foldin_result*, int64_t* offset, double* H);    /* n + 1 offsets, sub_size doubles (H may be NULL when 0) */
int fy_foldin_result_stats(const fy_foldin_result*, fy_foldin_stats* out);
void fy_foldin_result_free(fy_foldin_result*);
void fy_foldin_destroy(fy_foldin*);

#ifdef __cplusplus
}
#endif
#endif /* FILMYOU_H */
