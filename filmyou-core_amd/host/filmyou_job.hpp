// filmyou_job.hpp -- C++ host side of the drop-in (header only, C++17), a mirror of the reference's job interface over
// the C ABI of include/filmyou.h.  The reference's host language is Java; this image has no JVM, so the host layer is
// written in C++ (and mirrored in Python, filmyou-core_amd/host.py).  Names, argument meaning and error behaviour
// follow the reference:
//   fy::host::Configuration   <- org.apache.hadoop.conf.Configuration with the option names of
//                                M/rmrecommender/RMRecommenderDriver.java:49-120 (string values, typed getters)
//   fy::host::RM2Job::run     <- es.udc.fi.dc.irlab.rm.RM2Job.run (M/rm/RM2Job.java:76-100): returns 0 on success,
//                                throws std::runtime_error("RM2 failed!: ...") like RM2Job.java:144-147
//   fy::host::RowSimilarityJob::run <- Mahout RowSimilarityJob as invoked at
//                                M/baselinerecommender/BaselineRecommenderJob.java:241-253 (same option names)
//   fy::host::BaselineRecommenderJob::run <- the job around it (BaselineRecommenderJob.java:179-328), with usersFile, itemsFile,
//                                ratingShift and outputPathForSimilarityMatrix
// Input/output stay in the caller's hands (the reference's Cassandra / HDFS readers and writers are unchanged): the
// job takes rating triples and hands back rows through a sink callback shaped like writePreference
// (M/rm/AbstractRM2Reducer.java:404-406).
#pragma once
#include <cctype>
#include <cmath>
#include <cstdint>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/filmyou.h"

namespace fy {
namespace host {

class Configuration {
   public:
    void set(const std::string& k, const std::string& v) { kv_[k] = v; }
    void setInt(const std::string& k, long v) { kv_[k] = std::to_string(v); }
    void setBoolean(const std::string& k, bool v) { kv_[k] = v ? "true" : "false"; }
    bool has(const std::string& k) const { return kv_.count(k) || defaults().count(k); }
    std::string get(const std::string& k, const std::string& dflt = "") const {
        auto it = kv_.find(k);
        if (it != kv_.end()) return it->second;
        auto d = defaults().find(k);
        return d != defaults().end() ? d->second : dflt;
    }
    long getInt(const std::string& k, long dflt) const { return has(k) ? std::stol(get(k)) : dflt; }
    double getDouble(const std::string& k, double dflt) const { return has(k) ? std::stod(get(k)) : dflt; }
    bool getBoolean(const std::string& k, bool dflt) const { return has(k) ? get(k) == "true" : dflt; }

   private:
    // RMRecommenderDriver.loadDefaultSetup (M/rmrecommender/RMRecommenderDriver.java:89-120)
    static const std::map<std::string, std::string>& defaults() {
        static const std::map<std::string, std::string> d = {
            {"lambda", "0.1"}, {"numberOfRecommendations", "1000"}, {"clusterSplit", "400"}, {"splitSize", "100"},
            {"filterUsers", "0"}, {"directory", "recommendation"}, {"clustering", "clustering"},
            {"clusteringCount", "clusteringCount"}};
        return d;
    }
    std::map<std::string, std::string> kv_;
};

struct Ratings {   // what the reference's mappers receive: (user, item, score) records
    std::vector<int32_t> user, item;
    std::vector<float> score;
    void add(int32_t u, int32_t i, float s) { user.push_back(u); item.push_back(i); score.push_back(s); }
};

struct Clustering {   // the `clustering` and `clusteringCount` side files
    std::vector<int32_t> user, cluster;
    std::vector<int32_t> count;   // optional, numberOfClusters entries
};

// A batch of writes against the ratings table, in order (fy_ratings_apply): put = INSERT / UPDATE of (user, item), del = DELETE.
struct Writes {
    std::vector<int32_t> user, item;
    std::vector<float> score;
    std::vector<uint8_t> remove;
    void put(int32_t u, int32_t i, float s) { user.push_back(u); item.push_back(i); score.push_back(s); remove.push_back(0); }
    void del(int32_t u, int32_t i) { user.push_back(u); item.push_back(i); score.push_back(0.0f); remove.push_back(1); }
};

// The ratings after the batch, with the table's semantics (include/filmyou.h: the last write per key counts, survivors in source
// order, then the live writes in batch order): context, ratings, fy_ratings_apply, the COO copied back.  A host that keeps its
// fy_ratings resident calls fy_ratings_apply itself and never moves the old ratings; this mirror works on host records like the
// job classes below.  Throws std::runtime_error("applyWrites failed!: ...").
inline Ratings applyWrites(const Ratings& source, const Writes& w, fy_ratings_update_stats* stats = nullptr, int device = 0) {
    fy_context* ctx = nullptr;
    fy_ratings *src = nullptr, *upd = nullptr;
    auto fail = [&](const char* what) {
        const std::string msg = std::string("applyWrites failed!: ") + what + ": " + fy_last_error();
        if (upd) fy_ratings_destroy(upd);
        if (src) fy_ratings_destroy(src);
        if (ctx) fy_context_destroy(ctx);
        throw std::runtime_error(msg);
    };
    if (w.item.size() != w.user.size() || w.score.size() != w.user.size() || w.remove.size() != w.user.size())
        throw std::invalid_argument("applyWrites: the arrays of the batch differ in length");
    if (fy_context_create(device, &ctx) != FY_OK) fail("context");
    if (fy_ratings_create(ctx, (int64_t)source.user.size(), source.user.data(), source.item.data(), source.score.data(), FY_HOST, &src) != FY_OK) fail("ratings");
    if (fy_ratings_apply(ctx, src, (int64_t)w.user.size(), w.user.data(), w.item.data(), w.score.data(), w.remove.data(), FY_HOST, &upd, stats) != FY_OK)
        fail("apply");
    Ratings out;
    const size_t n = (size_t)fy_ratings_nnz(upd);
    out.user.resize(n); out.item.resize(n); out.score.resize(n);
    if (fy_ratings_copy_out(upd, out.user.data(), out.item.data(), out.score.data()) != FY_OK) fail("copy_out");
    fy_ratings_destroy(upd);
    fy_ratings_destroy(src);
    fy_context_destroy(ctx);
    return out;
}

// The hold-out split of host records (fy_ratings_holdout): {train, test}, both in source order; a rating's side is a hash of its
// (user, item) and the seed alone.  Like applyWrites this mirror moves records; a host that keeps its fy_ratings resident calls
// fy_ratings_holdout itself.  Throws std::runtime_error("holdout failed!: ...").
inline std::pair<Ratings, Ratings> holdout(const Ratings& source, double fraction, uint64_t seed = 0, int device = 0) {
    fy_context* ctx = nullptr;
    fy_ratings *src = nullptr, *part[2] = {nullptr, nullptr};
    auto release = [&]() {
        for (fy_ratings* p : part) fy_ratings_destroy(p);
        fy_ratings_destroy(src);
        if (ctx) fy_context_destroy(ctx);
    };
    auto fail = [&](const char* what) {
        const std::string msg = std::string("holdout failed!: ") + what + ": " + fy_last_error();
        release();
        throw std::runtime_error(msg);
    };
    if (fy_context_create(device, &ctx) != FY_OK) fail("context");
    if (fy_ratings_create(ctx, (int64_t)source.user.size(), source.user.data(), source.item.data(), source.score.data(), FY_HOST, &src) != FY_OK) fail("ratings");
    if (fy_ratings_holdout(ctx, src, fraction, seed, &part[0], &part[1]) != FY_OK) fail("split");
    std::pair<Ratings, Ratings> out;
    Ratings* side[2] = {&out.first, &out.second};
    for (int k = 0; k < 2; k++) {
        const size_t n = (size_t)fy_ratings_nnz(part[k]);
        side[k]->user.resize(n); side[k]->item.resize(n); side[k]->score.resize(n);
        if (fy_ratings_copy_out(part[k], side[k]->user.data(), side[k]->item.data(), side[k]->score.data()) != FY_OK) fail("copy_out");
    }
    release();
    return out;
}

// Ranking metrics of list results where they lie in HBM (fy_eval_*; include/filmyou.h states the definitions): prepared once from
// the test records on the caller's context, evaluate() takes any list result of that context.  The sums of fy_eval_sums are SUMS
// over the evaluated lists; the mean* accessors divide by users_evaluated, or by relevant_users with countMissing (users with
// relevant test items and no list then count as zeros).
class Evaluator {
   public:
    Evaluator(fy_context* ctx, const Ratings& test, const std::vector<int32_t>& cutoffs = {10}, double relevanceThreshold = 4.0,
              int gain = FY_EVAL_GAIN_BINARY, bool coverage = false) {
        if (cutoffs.empty() || cutoffs.size() > FY_EVAL_MAX_CUTOFFS) throw std::invalid_argument("Evaluator: 1 to 8 cutoffs");
        fy_eval_params p{};
        p.n_cutoffs = (int32_t)cutoffs.size();
        for (size_t k = 0; k < cutoffs.size(); k++) p.cutoffs[k] = cutoffs[k];
        p.gain = gain;
        p.flags = coverage ? FY_EVAL_COVERAGE : 0u;
        p.relevance_threshold = relevanceThreshold;
        fy_ratings* t = nullptr;
        if (fy_ratings_create(ctx, (int64_t)test.user.size(), test.user.data(), test.item.data(), test.score.data(), FY_HOST, &t) != FY_OK)
            throw std::runtime_error(std::string("Evaluator failed!: test ratings: ") + fy_last_error());
        const int rc = fy_eval_prepare(ctx, &p, t, &eval_);
        fy_ratings_destroy(t);      // the evaluator owns its tables
        if (rc != FY_OK) throw std::runtime_error(std::string("Evaluator failed!: ") + fy_last_error());
    }
    Evaluator(const Evaluator&) = delete;
    Evaluator& operator=(const Evaluator&) = delete;
    ~Evaluator() { fy_eval_destroy(eval_); }      // before its context

    fy_eval_sums evaluate(fy_result* lists, std::vector<int32_t>* perUserId = nullptr, std::vector<double>* perUser = nullptr) const {
        fy_eval_sums s{};
        if (perUserId || perUser) {     // `lists` is at most the row count
            const size_t rows = (size_t)fy_result_size(lists);
            if (perUserId) perUserId->assign(rows, 0);
            if (perUser) perUser->assign(rows * 5 * FY_EVAL_MAX_CUTOFFS, 0.0);
        }
        if (fy_eval_lists(eval_, lists, &s, perUserId ? perUserId->data() : nullptr, perUser ? perUser->data() : nullptr) != FY_OK)
            throw std::runtime_error(std::string("Evaluator failed!: ") + fy_last_error());
        if (perUserId) perUserId->resize((size_t)s.lists);
        if (perUser) perUser->resize((size_t)s.lists * 5 * (size_t)s.n_cutoffs);
        return s;
    }
    static double users(const fy_eval_sums& s, bool countMissing) { return (double)(countMissing ? s.relevant_users : s.users_evaluated); }
    static double meanPrecision(const fy_eval_sums& s, int c, bool countMissing = false) { return (double)s.hits[c] / ((double)s.cutoffs[c] * users(s, countMissing)); }
    static double meanRecall(const fy_eval_sums& s, int c, bool countMissing = false) { return s.recall[c] / users(s, countMissing); }
    static double meanAP(const fy_eval_sums& s, int c, bool countMissing = false) { return s.ap[c] / users(s, countMissing); }
    static double meanRR(const fy_eval_sums& s, int c, bool countMissing = false) { return s.rr[c] / users(s, countMissing); }
    static double meanNDCG(const fy_eval_sums& s, int c, bool countMissing = false) { return s.ndcg[c] / users(s, countMissing); }

   private:
    fy_eval* eval_ = nullptr;
};

// Rating-error sums of an estimates result (BaselineRecommenderJob::estimatePairs) against the true scores (fy_eval_estimates;
// Mahout's AverageAbsoluteDifferenceRecommenderEvaluator / RMSRecommenderEvaluator): record r of `truth` is the pair of row
// pair_offset + r of the estimates.  clamp = {lo, hi} clamps every estimate first.  SUMS; mae / rmse / coverage divide them.
// Throws std::runtime_error("estimateErrors failed!: ...").
inline fy_eval_errors estimateErrors(fy_context* ctx, fy_result* estimates, const Ratings& truth, const double* clamp = nullptr) {
    fy_ratings* t = nullptr;
    if (fy_ratings_create(ctx, (int64_t)truth.user.size(), truth.user.data(), truth.item.data(), truth.score.data(), FY_HOST, &t) != FY_OK)
        throw std::runtime_error(std::string("estimateErrors failed!: truth ratings: ") + fy_last_error());
    fy_eval_error_params p{};
    if (clamp) { p.has_clamp = 1; p.clamp_lo = clamp[0]; p.clamp_hi = clamp[1]; }
    fy_eval_errors e{};
    const int rc = fy_eval_estimates(ctx, estimates, t, &p, &e);
    fy_ratings_destroy(t);
    if (rc != FY_OK) throw std::runtime_error(std::string("estimateErrors failed!: ") + fy_last_error());
    return e;
}
inline double mae(const fy_eval_errors& e) { return e.sum_abs / (double)e.estimated; }
inline double rmse(const fy_eval_errors& e) { return std::sqrt(e.sum_sq / (double)e.estimated); }
inline double coverage(const fy_eval_errors& e) { return (double)e.estimated / (double)e.pairs; }

// The smoothing of the user language model (include/filmyou.h, FY_RM2_SMOOTHING_*) from the Configuration keys `smoothing` (jm --
// the default, parameter `lambda` --, dirichlet with `mu`, absoluteDiscounting with `delta`; case does not matter) into
// fy_rm2_params::flags and ::lambda.  mu / delta have no default; an unknown name or a missing parameter is std::invalid_argument.
// Next to it the estimator: `relevanceModel` = rm2 (the default) or rm1 (FY_RM2_ESTIMATOR_RM1), refused the same way.
inline void setSmoothing(const Configuration& conf, fy_rm2_params& p) {
    std::string name = conf.get("smoothing", "jm");
    for (char& ch : name) ch = (char)std::tolower((unsigned char)ch);
    const char* key = "lambda";   // Double.valueOf(conf.get("lambda")), AbstractRM2Reducer.java:108
    if (name == "dirichlet") { p.flags |= FY_RM2_SMOOTHING_DIRICHLET; key = "mu"; }
    else if (name == "absolutediscounting") { p.flags |= FY_RM2_SMOOTHING_ABSOLUTE_DISCOUNT; key = "delta"; }
    else if (name != "jm") throw std::invalid_argument("smoothing must be jm, dirichlet or absoluteDiscounting (got " + conf.get("smoothing") + ")");
    if (!conf.has(key)) throw std::invalid_argument("smoothing=" + name + " needs " + key);
    p.lambda = std::stod(conf.get(key));
    // relevanceModel = rm2 (the default, the reference's estimator) | rm1 (FY_RM2_ESTIMATOR_RM1); case does not matter
    std::string model = conf.get("relevanceModel", "rm2");
    for (char& ch : model) ch = (char)std::tolower((unsigned char)ch);
    if (model == "rm1") p.flags |= FY_RM2_ESTIMATOR_RM1;
    else if (model != "rm2") throw std::invalid_argument("relevanceModel must be rm2 or rm1 (got " + conf.get("relevanceModel") + ")");
}

// writePreference(context, userId, itemId, score, cluster)
using PreferenceSink = std::function<void(int32_t user, int32_t item, float score, int32_t cluster)>;

class RM2Job {
   public:
    explicit RM2Job(const Configuration& conf) : conf_(conf) {}

    // rm2/userSum and rm2/itemColl of the last run (what TestHDFSRM2.java:70-71 asserts)
    std::vector<int32_t> userSumKeys, itemCollKeys;
    std::vector<double> userSum, itemColl;
    double totalSum = 0.0;
    fy_stats stats{};

    int run(const Ratings& r, const Clustering& c, const PreferenceSink& sink) {
        fy_rm2_params p{};
        setSmoothing(conf_, p);
        p.number_of_items = (int32_t)conf_.getInt("numberOfItems", -1);
        p.number_of_clusters = (int32_t)conf_.getInt("numberOfClusters", -1);
        if (p.number_of_items <= 0 || p.number_of_clusters <= 0)
            throw std::invalid_argument("numberOfItems and numberOfClusters are required");
        p.number_of_recommendations = (int32_t)conf_.getInt("numberOfRecommendations", 1000);
        p.filter_users = (int32_t)conf_.getInt("filterUsers", 0);
        p.rank = 0;
        p.world = 1;
        std::vector<int32_t> cc;
        if (!c.count.empty()) {
            cc.assign((size_t)p.number_of_clusters, 0);
            for (size_t k = 0; k < c.count.size() && k < cc.size(); k++) cc[k] = c.count[k];
        }
        fy_result* res = nullptr;
        const int rc = fy_rm2_run(&p, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(),
                                  (int64_t)c.user.size(), c.user.data(), c.cluster.data(), cc.empty() ? nullptr : cc.data(), &res);
        if (rc != FY_OK) throw std::runtime_error(std::string("RM2 failed!: ") + fy_last_error());
        const int64_t n = fy_result_size(res);
        const int32_t *u = fy_result_key0(res), *i = fy_result_key1(res), *cl = fy_result_aux(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(u[k], i[k], s[k], cl[k]);
        const int64_t nu = fy_result_n_users(res), ni = fy_result_n_items(res);
        userSumKeys.assign(fy_result_user_id(res), fy_result_user_id(res) + nu);
        userSum.assign(fy_result_user_sum(res), fy_result_user_sum(res) + nu);
        itemCollKeys.assign(fy_result_item_id(res), fy_result_item_id(res) + ni);
        itemColl.assign(fy_result_item_coll(res), fy_result_item_coll(res) + ni);
        totalSum = fy_result_total_sum(res);
        fy_result_stats(res, &stats);
        fy_result_free(res);
        return 0;
    }

    // One rank of a multi-GPU job (one process per GPU): the staged entry points with the library's compiled RCCL transport
    // (fy_rccl_*, csrc/fy_rccl.hip).  `rccl_id` = the 128 bytes rank 0 got from fy_rccl_unique_id and handed to the other
    // ranks through the host's own channel (a Hadoop Configuration entry, a file, ...).  Emits this rank's users only.
    int runRank(const Ratings& r, const Clustering& c, const PreferenceSink& sink, int device, int rank, int world, const char* rccl_id) {
        fy_rm2_params p = params();
        p.rank = rank;
        p.world = world;
        fy_context* ctx = nullptr;
        fy_ratings* rt = nullptr;
        fy_rm2_job* job = nullptr;
        fy_rccl* comm = nullptr;
        fy_result* res = nullptr;
        auto fail = [&](const char* what) {
            const std::string msg = std::string("RM2 failed!: ") + what + ": " + fy_last_error();
            if (job) fy_rm2_job_destroy(job);
            if (comm) fy_rccl_destroy(comm);
            if (rt) fy_ratings_destroy(rt);
            if (ctx) fy_context_destroy(ctx);
            throw std::runtime_error(msg);
        };
        std::vector<int32_t> cc = counts(c, p.number_of_clusters);
        if (fy_context_create(device, &ctx) != FY_OK) fail("context");
        if (fy_ratings_create(ctx, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(), FY_HOST, &rt) != FY_OK) fail("ratings");
        if (fy_rm2_prepare(ctx, &p, rt, (int64_t)c.user.size(), c.user.data(), c.cluster.data(), cc.empty() ? nullptr : cc.data(), &job) != FY_OK) fail("prepare");
        if (fy_rccl_create(ctx, rank, world, rccl_id, &comm) != FY_OK) fail("rccl");
        fy_collectives coll{};
        if (fy_rccl_collectives(comm, &coll) != FY_OK || fy_rm2_set_collectives(job, &coll) != FY_OK) fail("collectives");
        if (fy_rm2_score(job, &res) != FY_OK) fail("score");
        collect(res, sink);
        fy_rccl_counters(comm, &allGathers, &reduceScatters, &collectiveBytes);
        fy_result_free(res);
        fy_rm2_job_destroy(job);
        fy_rccl_destroy(comm);
        fy_ratings_destroy(rt);
        fy_context_destroy(ctx);
        return 0;
    }
    int64_t allGathers = 0, reduceScatters = 0, collectiveBytes = 0;   // of the last runRank

    // run() with the lists evaluated where they lie, before they are downloaded for the sink: one context, the staged entry points,
    // an Evaluator prepared from `test` (cutoffs, relevanceThreshold, gain as in fy::host::Evaluator).  evaluation holds the sums.
    fy_eval_sums evaluation{};
    int runEvaluated(const Ratings& r, const Clustering& c, const Ratings& test, const std::vector<int32_t>& cutoffs, double relevanceThreshold,
                     const PreferenceSink& sink, int gain = FY_EVAL_GAIN_BINARY, int device = 0) {
        fy_rm2_params p = params();
        fy_context* ctx = nullptr;
        fy_ratings* rt = nullptr;
        fy_rm2_job* job = nullptr;
        fy_result* res = nullptr;
        auto release = [&]() {
            if (res) fy_result_free(res);
            if (job) fy_rm2_job_destroy(job);
            if (rt) fy_ratings_destroy(rt);
            if (ctx) fy_context_destroy(ctx);
        };
        auto fail = [&](const char* what) {
            const std::string msg = std::string("RM2 failed!: ") + what + ": " + fy_last_error();
            release();
            throw std::runtime_error(msg);
        };
        std::vector<int32_t> cc = counts(c, p.number_of_clusters);
        if (fy_context_create(device, &ctx) != FY_OK) fail("context");
        if (fy_ratings_create(ctx, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(), FY_HOST, &rt) != FY_OK) fail("ratings");
        if (fy_rm2_prepare(ctx, &p, rt, (int64_t)c.user.size(), c.user.data(), c.cluster.data(), cc.empty() ? nullptr : cc.data(), &job) != FY_OK) fail("prepare");
        if (fy_rm2_score(job, &res) != FY_OK) fail("score");
        try {
            Evaluator ev(ctx, test, cutoffs, relevanceThreshold, gain);
            evaluation = ev.evaluate(res);
        } catch (...) {
            release();
            throw;
        }
        collect(res, sink);
        release();
        return 0;
    }

    // RM2 on request (fy_rm2_score_users): the lists of the listed raw user ids alone, with the work sized by the request --
    // "usersFile" of the Python host.  `users` empty = read the configuration key usersFile (one id per line, fy_idfile_read).
    // One GPU: context, ratings, prepare, the request.  requestStats holds what the request touched.
    fy_rm2_request_stats requestStats{};
    int runUsers(const Ratings& r, const Clustering& c, std::vector<int32_t> users, const PreferenceSink& sink, int device = 0) {
        fy_rm2_params p = params();
        if (users.empty() && conf_.has("usersFile")) {
            int64_t n = 0;
            int32_t* ids = nullptr;
            if (fy_idfile_read(conf_.get("usersFile").c_str(), &n, &ids) != FY_OK) throw std::runtime_error(std::string("RM2 failed!: ") + fy_last_error());
            users.assign(ids, ids + n);
            fy_buffer_free(ids);
        }
        fy_context* ctx = nullptr;
        fy_ratings* rt = nullptr;
        fy_rm2_job* job = nullptr;
        fy_result* res = nullptr;
        auto fail = [&](const char* what) {
            const std::string msg = std::string("RM2 failed!: ") + what + ": " + fy_last_error();
            if (job) fy_rm2_job_destroy(job);
            if (rt) fy_ratings_destroy(rt);
            if (ctx) fy_context_destroy(ctx);
            throw std::runtime_error(msg);
        };
        std::vector<int32_t> cc = counts(c, p.number_of_clusters);
        if (fy_context_create(device, &ctx) != FY_OK) fail("context");
        if (fy_ratings_create(ctx, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(), FY_HOST, &rt) != FY_OK) fail("ratings");
        if (fy_rm2_prepare(ctx, &p, rt, (int64_t)c.user.size(), c.user.data(), c.cluster.data(), cc.empty() ? nullptr : cc.data(), &job) != FY_OK) fail("prepare");
        const fy_rm2_request rq{(int64_t)users.size(), users.data()};
        if (fy_rm2_score_users(job, &rq, &res) != FY_OK) fail("score_users");
        const int64_t n = fy_result_size(res);
        const int32_t *u = fy_result_key0(res), *i = fy_result_key1(res), *cl = fy_result_aux(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(u[k], i[k], s[k], cl[k]);
        fy_result_stats(res, &stats);
        fy_result_request_stats(res, &requestStats);
        fy_result_free(res);
        fy_rm2_job_destroy(job);
        fy_ratings_destroy(rt);
        fy_context_destroy(ctx);
        return 0;
    }

    // RM2 for item sets handed in (fy_rm2_score_profiles): an anonymous or new visitor's whole profile scored as one more member of
    // a cluster (resident = false: cluster[p] names it), or a resident user's row with pending writes applied (resident = true: the
    // label is the user id, the cluster is that user's).  Profile p holds the entries start[p] .. start[p + 1], applied in order; the
    // last entry per item counts; a non-zero remove, or a score that is not > 0, removes the item.  The job stays as prepared: one
    // GPU, context, ratings, prepare, the call.  Rows reach the sink grouped by profile in the order given, the label in the user
    // column.  profileStats holds the counters.
    struct Profiles {
        std::vector<int32_t> label, cluster;
        std::vector<int64_t> start{0};
        std::vector<int32_t> item;
        std::vector<float> score;
        std::vector<uint8_t> remove;
        bool resident = false;
        void begin(int32_t l, int32_t c = 0) { label.push_back(l); cluster.push_back(c); start.push_back(start.back()); }      // then put / del
        void put(int32_t i, float s) { item.push_back(i); score.push_back(s); remove.push_back(0); start.back()++; }
        void del(int32_t i) { item.push_back(i); score.push_back(0.0f); remove.push_back(1); start.back()++; }
    };
    fy_rm2_profile_stats profileStats{};
    int scoreProfiles(const Ratings& r, const Clustering& c, const Profiles& profiles, const PreferenceSink& sink, int device = 0) {
        if (profiles.start.size() != profiles.label.size() + 1 || profiles.cluster.size() != profiles.label.size() ||
            profiles.item.size() != profiles.score.size() || profiles.item.size() != profiles.remove.size() ||
            (size_t)profiles.start.back() != profiles.item.size())
            throw std::invalid_argument("scoreProfiles: the arrays of the profiles differ in length");
        fy_rm2_params p = params();
        fy_context* ctx = nullptr;
        fy_ratings* rt = nullptr;
        fy_rm2_job* job = nullptr;
        fy_result* res = nullptr;
        auto fail = [&](const char* what) {
            const std::string msg = std::string("RM2 failed!: ") + what + ": " + fy_last_error();
            if (job) fy_rm2_job_destroy(job);
            if (rt) fy_ratings_destroy(rt);
            if (ctx) fy_context_destroy(ctx);
            throw std::runtime_error(msg);
        };
        std::vector<int32_t> cc = counts(c, p.number_of_clusters);
        if (fy_context_create(device, &ctx) != FY_OK) fail("context");
        if (fy_ratings_create(ctx, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(), FY_HOST, &rt) != FY_OK) fail("ratings");
        if (fy_rm2_prepare(ctx, &p, rt, (int64_t)c.user.size(), c.user.data(), c.cluster.data(), cc.empty() ? nullptr : cc.data(), &job) != FY_OK) fail("prepare");
        fy_rm2_profiles q{};
        q.n_profiles = (int64_t)profiles.label.size();
        q.user = profiles.label.empty() ? nullptr : profiles.label.data();
        q.start = profiles.start.data();
        q.item = profiles.item.empty() ? nullptr : profiles.item.data();
        q.score = profiles.item.empty() ? nullptr : profiles.score.data();
        q.remove = profiles.item.empty() ? nullptr : profiles.remove.data();
        q.cluster = profiles.cluster.empty() ? nullptr : profiles.cluster.data();
        q.base = profiles.resident ? FY_PROFILE_ON_RESIDENT : FY_PROFILE_WHOLE;
        q.rank = 0;
        q.world = 1;
        if (fy_rm2_score_profiles(job, &q, &res) != FY_OK) fail("score_profiles");
        const int64_t n = fy_result_size(res);
        const int32_t *u = fy_result_key0(res), *i = fy_result_key1(res), *cl = fy_result_aux(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(u[k], i[k], s[k], cl[k]);
        fy_result_stats(res, &stats);
        fy_result_rm2_profile_stats(res, &profileStats);
        fy_result_free(res);
        fy_rm2_job_destroy(job);
        fy_ratings_destroy(rt);
        fy_context_destroy(ctx);
        return 0;
    }

    // RM2Job.run on the reference's own files (M/rm/RM2Job.java:76-100 with useCassandraInput / Output = false): ratings from
    // <mapred.input.dir>, <directory>/<clustering>, <directory>/<clusteringCount>; writes <directory>/rm2/userSum,
    // <directory>/rm2/itemColl (MapFile) and the recommendations under <mapred.output.dir>.  Files: fy_seqfile_* (layout
    // parity unpinned, see csrc/fy_seqfile.cpp).  <directory>/rm2 is NOT wiped here (no filesystem walk in this header).
    int runFiles() {
        const std::string in = conf_.get("mapred.input.dir"), out = conf_.get("mapred.output.dir"), base = conf_.get("directory");
        if (in.empty() || out.empty()) throw std::invalid_argument("mapred.input.dir and mapred.output.dir are required");
        Ratings r;
        Clustering c;
        int64_t n = 0;
        int32_t *a = nullptr, *b = nullptr;
        float* v = nullptr;
        if (fy_seqfile_read_intpair_float(in.c_str(), &n, &a, &b, &v) != FY_OK) throw std::runtime_error(std::string("RM2 failed!: ") + fy_last_error());
        r.user.assign(a, a + n); r.item.assign(b, b + n); r.score.assign(v, v + n);
        fy_buffer_free(a); fy_buffer_free(b); fy_buffer_free(v);
        if (fy_seqfile_read_int_int((base + "/" + conf_.get("clustering")).c_str(), &n, &a, &b) != FY_OK)
            throw std::runtime_error(std::string("RM2 failed!: ") + fy_last_error());
        c.user.assign(a, a + n); c.cluster.assign(b, b + n);
        fy_buffer_free(a); fy_buffer_free(b);
        if (fy_seqfile_read_int_int((base + "/" + conf_.get("clusteringCount")).c_str(), &n, &a, &b) != FY_OK)
            throw std::runtime_error(std::string("RM2 failed!: ") + fy_last_error());
        const long K = conf_.getInt("numberOfClusters", -1);
        c.count.assign((size_t)(K > 0 ? K : 1), 0);
        for (int64_t k = 0; k < n; k++)
            if (a[k] >= 0 && a[k] < (int32_t)c.count.size()) c.count[(size_t)a[k]] = b[k];
        fy_buffer_free(a); fy_buffer_free(b);
        std::vector<int32_t> ou, oi;
        std::vector<float> os;
        run(r, c, [&](int32_t user, int32_t item, float score, int32_t) { ou.push_back(user); oi.push_back(item); os.push_back(score); });
        if (fy_seqfile_write_int_double((base + "/rm2/userSum/part-r-00000").c_str(), (int64_t)userSum.size(), userSumKeys.data(), userSum.data()) != FY_OK ||
            fy_mapfile_write_int_double((base + "/rm2/itemColl/part-r-00000").c_str(), (int64_t)itemColl.size(), itemCollKeys.data(), itemColl.data()) != FY_OK ||
            fy_seqfile_write_intpair_float((out + "/part-r-00000").c_str(), (int64_t)ou.size(), ou.data(), oi.data(), os.data()) != FY_OK)
            throw std::runtime_error(std::string("RM2 failed!: ") + fy_last_error());
        return 0;
    }

   private:
    fy_rm2_params params() const {
        fy_rm2_params p{};
        setSmoothing(conf_, p);
        p.number_of_items = (int32_t)conf_.getInt("numberOfItems", -1);
        p.number_of_clusters = (int32_t)conf_.getInt("numberOfClusters", -1);
        if (p.number_of_items <= 0 || p.number_of_clusters <= 0) throw std::invalid_argument("numberOfItems and numberOfClusters are required");
        p.number_of_recommendations = (int32_t)conf_.getInt("numberOfRecommendations", 1000);
        p.filter_users = (int32_t)conf_.getInt("filterUsers", 0);
        p.world = 1;
        return p;
    }
    static std::vector<int32_t> counts(const Clustering& c, int32_t K) {
        std::vector<int32_t> cc;
        if (!c.count.empty()) {
            cc.assign((size_t)K, 0);
            for (size_t k = 0; k < c.count.size() && k < cc.size(); k++) cc[k] = c.count[k];
        }
        return cc;
    }
    void collect(fy_result* res, const PreferenceSink& sink) {
        const int64_t n = fy_result_size(res);
        const int32_t *u = fy_result_key0(res), *i = fy_result_key1(res), *cl = fy_result_aux(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(u[k], i[k], s[k], cl[k]);
        const int64_t nu = fy_result_n_users(res), ni = fy_result_n_items(res);
        userSumKeys.assign(fy_result_user_id(res), fy_result_user_id(res) + nu);
        userSum.assign(fy_result_user_sum(res), fy_result_user_sum(res) + nu);
        itemCollKeys.assign(fy_result_item_id(res), fy_result_item_id(res) + ni);
        itemColl.assign(fy_result_item_coll(res), fy_result_item_coll(res) + ni);
        totalSum = fy_result_total_sum(res);
        fy_result_stats(res, &stats);
    }
    Configuration conf_;
};

class RowSimilarityJob {
   public:
    using SimilaritySink = std::function<void(int32_t item, int32_t other, float similarity)>;
    // --similarityClassname -> FY_SIMILARITY_*: a SIMILARITY_* name of Mahout's VectorSimilarityMeasures or the fully qualified
    // measure class, with or without the "class " that String.valueOf(X.class) puts in front (the reference's default value,
    // BaselineRecommenderJob.java:163)
    static int similarityId(std::string name) {
        static const struct { const char* name; const char* cls; int id; } table[] = {
            {"SIMILARITY_COSINE", "CosineSimilarity", FY_SIMILARITY_COSINE},
            {"SIMILARITY_COOCCURRENCE", "CooccurrenceCountSimilarity", FY_SIMILARITY_COOCCURRENCE},
            {"SIMILARITY_TANIMOTO_COEFFICIENT", "TanimotoCoefficientSimilarity", FY_SIMILARITY_TANIMOTO_COEFFICIENT},
            {"SIMILARITY_LOGLIKELIHOOD", "LoglikelihoodSimilarity", FY_SIMILARITY_LOGLIKELIHOOD},
            {"SIMILARITY_CITY_BLOCK", "CityBlockSimilarity", FY_SIMILARITY_CITY_BLOCK},
            {"SIMILARITY_EUCLIDEAN_DISTANCE", "EuclideanDistanceSimilarity", FY_SIMILARITY_EUCLIDEAN_DISTANCE},
            {"SIMILARITY_PEARSON_CORRELATION", "PearsonCorrelationSimilarity", FY_SIMILARITY_PEARSON_CORRELATION}};
        for (const auto& t : table)
            if (name == t.name) return t.id;
        const std::string cls = "class ", pkg = "org.apache.mahout.math.hadoop.similarity.cooccurrence.measures.";
        if (name.compare(0, cls.size(), cls) == 0) name.erase(0, cls.size());
        if (name.compare(0, pkg.size(), pkg) == 0)
            for (const auto& t : table)
                if (name.compare(pkg.size(), std::string::npos, t.cls) == 0) return t.id;
        throw std::invalid_argument("similarityClassname must be a SIMILARITY_* name or a measure class of " + pkg + "*");
    }
    // args as passed by BaselineRecommenderJob: --similarityClassname, --maxSimilaritiesPerRow,
    // --excludeSelfSimilarity, --threshold
    int run(const Ratings& r, const std::string& similarityClassname, int maxSimilaritiesPerRow, bool excludeSelfSimilarity,
            const double* threshold, const SimilaritySink& sink) {
        fy_itemsim_params p{};
        p.similarity = similarityId(similarityClassname);
        p.max_similarities_per_item = maxSimilaritiesPerRow;
        p.exclude_self = excludeSelfSimilarity ? 1 : 0;
        p.has_threshold = threshold ? 1 : 0;
        p.threshold = threshold ? *threshold : 0.0;
        p.rank = 0;
        p.world = 1;
        fy_result* res = nullptr;
        const int rc = fy_itemsim_run(&p, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(), &res);
        if (rc != FY_OK) throw std::runtime_error(std::string("RowSimilarityJob failed!: ") + fy_last_error());
        const int64_t n = fy_result_size(res);
        const int32_t *a = fy_result_key0(res), *b = fy_result_key1(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(a[k], b[k], s[k]);
        fy_result_free(res);
        return 0;
    }
    // The rows of the listed items alone (Mahout's ItemBasedRecommender.mostSimilarItems, one row each): fy_itemsim_prepare, one
    // fy_itemsim_rows request, everything released.  Unknown and repeated ids are passed over.  requestStats: what the request touched.
    fy_itemsim_request_stats requestStats{};
    int runItems(const Ratings& r, std::vector<int32_t> items, const std::string& similarityClassname, int maxSimilaritiesPerRow,
                 bool excludeSelfSimilarity, const double* threshold, const SimilaritySink& sink, int device = 0) {
        fy_itemsim_params p{};
        p.similarity = similarityId(similarityClassname);
        p.max_similarities_per_item = maxSimilaritiesPerRow;
        p.exclude_self = excludeSelfSimilarity ? 1 : 0;
        p.has_threshold = threshold ? 1 : 0;
        p.threshold = threshold ? *threshold : 0.0;
        p.rank = 0;
        p.world = 1;
        fy_context* ctx = nullptr;
        fy_ratings* rt = nullptr;
        fy_itemsim_job* job = nullptr;
        fy_result* res = nullptr;
        auto release = [&]() {
            fy_result_free(res);
            fy_itemsim_job_destroy(job);
            fy_ratings_destroy(rt);
            fy_context_destroy(ctx);
        };
        auto fail = [&](const char* what) {
            const std::string msg = std::string("RowSimilarityJob failed!: ") + what + ": " + fy_last_error();
            release();
            throw std::runtime_error(msg);
        };
        if (fy_context_create(device, &ctx) != FY_OK) fail("context");
        if (fy_ratings_create(ctx, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(), FY_HOST, &rt) != FY_OK) fail("ratings");
        if (fy_itemsim_prepare(ctx, &p, rt, &job) != FY_OK) fail("prepare");
        const fy_itemsim_request rq{(int64_t)items.size(), items.empty() ? nullptr : items.data()};
        if (fy_itemsim_rows(job, &rq, &res) != FY_OK) fail("rows");
        const int64_t n = fy_result_size(res);
        const int32_t *a = fy_result_key0(res), *b = fy_result_key1(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(a[k], b[k], s[k]);
        fy_result_itemsim_request_stats(res, &requestStats);
        release();
        return 0;
    }
};

// What BaselineRecommenderJob::prepare returns: a prepared similarity job and the context it lives on, owned (move-only).
class PreparedItemSimilarity {
   public:
    PreparedItemSimilarity() = default;
    PreparedItemSimilarity(const PreparedItemSimilarity&) = delete;
    PreparedItemSimilarity& operator=(const PreparedItemSimilarity&) = delete;
    PreparedItemSimilarity(PreparedItemSimilarity&& o) noexcept : ctx_(o.ctx_), job_(o.job_) { o.ctx_ = nullptr; o.job_ = nullptr; }
    PreparedItemSimilarity& operator=(PreparedItemSimilarity&& o) noexcept {
        if (this != &o) {
            close();
            ctx_ = o.ctx_; job_ = o.job_;
            o.ctx_ = nullptr; o.job_ = nullptr;
        }
        return *this;
    }
    ~PreparedItemSimilarity() { close(); }
    fy_itemsim_job* job() const { return job_; }
    fy_context* context() const { return ctx_; }
    void dropRows() { fy_itemsim_job_drop_rows(job_); }      // the row store; the job stays valid
    void close() {
        if (job_) fy_itemsim_job_destroy(job_);
        if (ctx_) fy_context_destroy(ctx_);
        job_ = nullptr;
        ctx_ = nullptr;
    }

   private:
    friend class BaselineRecommenderJob;
    fy_context* ctx_ = nullptr;
    fy_itemsim_job* job_ = nullptr;
};

// Item-based CF from the similarity phase on (M/baselinerecommender/BaselineRecommenderJob.java:179-328), with the job's option
// names: the similarity build, then the recommendation pass on one context.  usersFile / itemsFile (paths of one id per line; empty
// = not given, the reference's NULL), ratingShift and outputPathForSimilarityMatrix as in the reference (:74, 189, 259-278, 305-307;
// BaselineAggregateAndRecommendReducer.java:170-181, 209; BaselineToItemPrefsMapper.java:60).
class BaselineRecommenderJob {
   public:
    int numRecommendations = 100, maxPrefsPerUser = 50, maxSimilaritiesPerItem = 100;
    std::string similarityClassname = "SIMILARITY_COSINE";
    bool booleanData = false, hasThreshold = false;
    double threshold = 0.0;
    std::string usersFile, itemsFile, outputPathForSimilarityMatrix;
    float ratingShift = 0.0f;
    fy_stats stats{};   // of the recommendation pass

    using RecommendationSink = std::function<void(int32_t user, int32_t item, float score)>;

    int run(const Ratings& r, const RecommendationSink& sink, int device = 0) {
        fy_context* ctx = nullptr;
        fy_ratings *rt = nullptr, *shifted = nullptr;
        fy_result *sims = nullptr, *pairs = nullptr, *res = nullptr;
        int32_t *users = nullptr, *items = nullptr;
        auto release = [&]() {
            if (res) fy_result_free(res);
            if (pairs) fy_result_free(pairs);
            if (sims) fy_result_free(sims);
            if (shifted) fy_ratings_destroy(shifted);
            if (rt) fy_ratings_destroy(rt);
            if (ctx) fy_context_destroy(ctx);
            fy_buffer_free(users);
            fy_buffer_free(items);
        };
        auto fail = [&](const char* what) {
            const std::string msg = std::string("BaselineRecommenderJob failed!: ") + what + ": " + fy_last_error();
            release();
            throw std::runtime_error(msg);
        };
        fy_itemcf_filter f{};
        if (!usersFile.empty()) {
            f.has_users = 1;
            if (fy_idfile_read(usersFile.c_str(), &f.n_users, &users) != FY_OK) fail("usersFile");
            f.users = users;
        }
        if (!itemsFile.empty()) {
            f.has_items = 1;
            if (fy_idfile_read(itemsFile.c_str(), &f.n_items, &items) != FY_OK) fail("itemsFile");
            f.items = items;
        }
        fy_itemsim_params sp{};
        sp.similarity = RowSimilarityJob::similarityId(similarityClassname);
        sp.max_similarities_per_item = maxSimilaritiesPerItem;
        sp.exclude_self = 1;
        sp.has_threshold = hasThreshold ? 1 : 0;
        sp.threshold = threshold;
        sp.world = 1;
        sp.min_prefs_per_user = 1;
        fy_itemcf_params cp{};
        cp.num_recommendations = numRecommendations;
        cp.max_prefs_per_user = maxPrefsPerUser;
        cp.boolean_data = booleanData ? 1 : 0;
        cp.world = 1;
        if (fy_context_create(device, &ctx) != FY_OK) fail("context");
        if (fy_ratings_create(ctx, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(), FY_HOST, &rt) != FY_OK) fail("ratings");
        if (ratingShift != 0.0f && fy_ratings_shifted(ctx, rt, ratingShift, &shifted) != FY_OK) fail("ratingShift");
        const fy_ratings* prefs = shifted ? shifted : rt;
        if (fy_itemsim_build(ctx, &sp, prefs, &sims) != FY_OK) fail("similarity");
        if (!outputPathForSimilarityMatrix.empty()) {
            if (fy_itemsim_pairs(ctx, sims, &pairs) != FY_OK) fail("item pairs");
            if (fy_simpairs_write_text(outputPathForSimilarityMatrix.c_str(), fy_result_size(pairs), fy_result_key0(pairs),
                                       fy_result_key1(pairs), fy_result_value(pairs)) != FY_OK)
                fail("outputPathForSimilarityMatrix");
        }
        if (fy_itemcf_recommend_filtered(ctx, &cp, &f, prefs, sims, &res) != FY_OK) fail("recommend");
        const int64_t n = fy_result_size(res);
        const int32_t *u = fy_result_key0(res), *i = fy_result_key1(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(u[k], i[k], s[k]);
        fy_result_stats(res, &stats);
        release();
        return 0;
    }

    // "These users just rated something": prepare() keeps the similarity phase of run() as a prepared job (self-similarity excluded,
    // world 1, no input preparation, ratingShift applied first) on a context of its own and returns the handle that owns both;
    // recommendUsers() then answers any number of requests on it with the lists run() with that usersFile would emit
    // (fy_itemcf_recommend_prepared; itemsFile, numRecommendations, maxPrefsPerUser and booleanData are read at each request).  The
    // similarity rows a request builds stay on the prepared job for the next one (dropRows releases them).  After a write, prepare
    // again on the new ratings.
    fy_itemcf_request_stats requestStats{};
    PreparedItemSimilarity prepare(const Ratings& r, int device = 0) const {
        PreparedItemSimilarity p;
        fy_ratings *rt = nullptr, *shifted = nullptr;
        auto fail = [&](const char* what) {
            const std::string msg = std::string("BaselineRecommenderJob failed!: ") + what + ": " + fy_last_error();
            if (shifted) fy_ratings_destroy(shifted);
            if (rt) fy_ratings_destroy(rt);
            throw std::runtime_error(msg);      // (p goes with the unwinding)
        };
        fy_itemsim_params sp{};
        sp.similarity = RowSimilarityJob::similarityId(similarityClassname);
        sp.max_similarities_per_item = maxSimilaritiesPerItem;
        sp.exclude_self = 1;
        sp.has_threshold = hasThreshold ? 1 : 0;
        sp.threshold = threshold;
        sp.world = 1;
        sp.min_prefs_per_user = 1;
        if (fy_context_create(device, &p.ctx_) != FY_OK) fail("context");
        if (fy_ratings_create(p.ctx_, (int64_t)r.user.size(), r.user.data(), r.item.data(), r.score.data(), FY_HOST, &rt) != FY_OK) fail("ratings");
        if (ratingShift != 0.0f && fy_ratings_shifted(p.ctx_, rt, ratingShift, &shifted) != FY_OK) fail("ratingShift");
        if (fy_itemsim_prepare(p.ctx_, &sp, shifted ? shifted : rt, &p.job_) != FY_OK) fail("prepare");
        if (shifted) fy_ratings_destroy(shifted);      // the prepared job owns what it needs
        fy_ratings_destroy(rt);
        return p;
    }
    int recommendUsers(PreparedItemSimilarity& prepared, const std::vector<int32_t>& users, const RecommendationSink& sink) {
        if (!prepared.job()) throw std::runtime_error("BaselineRecommenderJob failed!: recommendUsers on a closed prepared job");
        fy_result* res = nullptr;
        int32_t* items = nullptr;
        auto fail = [&](const char* what) {
            const std::string msg = std::string("BaselineRecommenderJob failed!: ") + what + ": " + fy_last_error();
            if (res) fy_result_free(res);
            fy_buffer_free(items);
            throw std::runtime_error(msg);
        };
        fy_itemcf_filter f{};
        f.has_users = 1;
        f.n_users = (int64_t)users.size();
        f.users = users.empty() ? nullptr : users.data();
        if (!itemsFile.empty()) {
            f.has_items = 1;
            if (fy_idfile_read(itemsFile.c_str(), &f.n_items, &items) != FY_OK) fail("itemsFile");
            f.items = items;
        }
        fy_itemcf_params cp{};
        cp.num_recommendations = numRecommendations;
        cp.max_prefs_per_user = maxPrefsPerUser;
        cp.boolean_data = booleanData ? 1 : 0;
        cp.world = 1;
        if (fy_itemcf_recommend_prepared(prepared.job(), &cp, &f, &res) != FY_OK) fail("recommend");
        const int64_t n = fy_result_size(res);
        const int32_t *u = fy_result_key0(res), *i = fy_result_key1(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(u[k], i[k], s[k]);
        fy_result_stats(res, &stats);
        fy_result_itemcf_request_stats(res, &requestStats);
        fy_result_free(res);
        fy_buffer_free(items);
        return 0;
    }

    // "This visitor has no row yet" / "what if I rated this": the lists of recommendUsers for preference vectors handed in
    // (fy_itemcf_recommend_profiles) on the standing prepared job and its warm row store; the similarity rows stay as prepared.
    // Profile p holds the entries start[p] .. start[p + 1]; the last entry per item counts, a non-zero remove deletes the item.
    // resident = false: whole profiles (the label only names the rows); true: applied on top of the prepared row of user label[p].
    // Scores are taken as the job's ratings hold them: ratingShift is added here (fp32) as prepare() adds it to the ratings.
    struct Profiles {
        std::vector<int32_t> label;
        std::vector<int64_t> start{0};
        std::vector<int32_t> item;
        std::vector<float> score;
        std::vector<uint8_t> remove;
        bool resident = false;
        void begin(int32_t l) { label.push_back(l); start.push_back(start.back()); }      // then put / del into the profile begun last
        void put(int32_t i, float s) { item.push_back(i); score.push_back(s); remove.push_back(0); start.back()++; }
        void del(int32_t i) { item.push_back(i); score.push_back(0.0f); remove.push_back(1); start.back()++; }
    };
    fy_itemcf_profile_stats profileStats{};
    int recommendProfiles(PreparedItemSimilarity& prepared, const Profiles& profiles, const RecommendationSink& sink) {
        if (!prepared.job()) throw std::runtime_error("BaselineRecommenderJob failed!: recommendProfiles on a closed prepared job");
        if (profiles.start.size() != profiles.label.size() + 1 || profiles.item.size() != profiles.score.size() ||
            profiles.item.size() != profiles.remove.size() || (size_t)profiles.start.back() != profiles.item.size())
            throw std::invalid_argument("recommendProfiles: the arrays of the profiles differ in length");
        fy_result* res = nullptr;
        int32_t* items = nullptr;
        auto fail = [&](const char* what) {
            const std::string msg = std::string("BaselineRecommenderJob failed!: ") + what + ": " + fy_last_error();
            if (res) fy_result_free(res);
            fy_buffer_free(items);
            throw std::runtime_error(msg);
        };
        std::vector<float> shifted;
        if (ratingShift != 0.0f) {
            shifted = profiles.score;
            for (float& v : shifted) v = v + ratingShift;
        }
        fy_itemcf_profiles q{};
        q.n_profiles = (int64_t)profiles.label.size();
        q.user = profiles.label.empty() ? nullptr : profiles.label.data();
        q.start = profiles.start.data();
        q.item = profiles.item.empty() ? nullptr : profiles.item.data();
        q.score = profiles.item.empty() ? nullptr : (ratingShift != 0.0f ? shifted.data() : profiles.score.data());
        q.remove = profiles.item.empty() ? nullptr : profiles.remove.data();
        q.base = profiles.resident ? FY_PROFILE_ON_RESIDENT : FY_PROFILE_WHOLE;
        fy_itemcf_filter f{};
        if (!itemsFile.empty()) {
            f.has_items = 1;
            if (fy_idfile_read(itemsFile.c_str(), &f.n_items, &items) != FY_OK) fail("itemsFile");
            f.items = items;
        }
        fy_itemcf_params cp{};
        cp.num_recommendations = numRecommendations;
        cp.max_prefs_per_user = maxPrefsPerUser;
        cp.boolean_data = booleanData ? 1 : 0;
        cp.world = 1;
        if (fy_itemcf_recommend_profiles(prepared.job(), &cp, &q, &f, &res) != FY_OK) fail("recommend profiles");
        const int64_t n = fy_result_size(res);
        const int32_t *u = fy_result_key0(res), *i = fy_result_key1(res);
        const float* s = fy_result_value(res);
        for (int64_t k = 0; k < n; k++) sink(u[k], i[k], s[k]);
        fy_result_stats(res, &stats);
        fy_result_itemcf_profile_stats(res, &profileStats);
        fy_result_free(res);
        fy_buffer_free(items);
        return 0;
    }

    // "What would this user give this item": the cell (user, item) of the pass recommendUsers runs, before the top-N
    // (fy_itemcf_estimate_prepared; maxPrefsPerUser and booleanData are read at each call).  One row per pair in the order given:
    // the sink (may be empty) receives (user, item, estimate, FY_ESTIMATE_* status), the estimate is NaN unless the status is
    // FY_ESTIMATE_OK.  Returns the result, which lives on prepared.context() -- estimateErrors takes it -- and is the caller's to
    // release with fy_result_free before the prepared job is closed.
    using EstimateSink = std::function<void(int32_t user, int32_t item, float estimate, int32_t status)>;
    fy_itemcf_estimate_stats estimateStats{};
    fy_result* estimatePairs(PreparedItemSimilarity& prepared, const std::vector<int32_t>& users, const std::vector<int32_t>& items,
                             const EstimateSink& sink = nullptr) {
        if (!prepared.job()) throw std::runtime_error("BaselineRecommenderJob failed!: estimatePairs on a closed prepared job");
        if (users.size() != items.size()) throw std::invalid_argument("estimatePairs: users and items differ in length");
        fy_itemcf_params cp{};
        cp.max_prefs_per_user = maxPrefsPerUser;
        cp.boolean_data = booleanData ? 1 : 0;
        cp.world = 1;
        fy_itemcf_pairs q{};
        q.n_pairs = (int64_t)users.size();
        q.users = users.empty() ? nullptr : users.data();
        q.items = items.empty() ? nullptr : items.data();
        q.location = FY_HOST;
        fy_result* res = nullptr;
        if (fy_itemcf_estimate_prepared(prepared.job(), &cp, &q, &res) != FY_OK)
            throw std::runtime_error(std::string("BaselineRecommenderJob failed!: estimate: ") + fy_last_error());
        if (sink) {
            const int64_t n = fy_result_size(res);
            const int32_t *u = fy_result_key0(res), *i = fy_result_key1(res), *st = fy_result_aux(res);
            const float* v = fy_result_value(res);
            for (int64_t k = 0; k < n; k++) sink(u[k], i[k], v[k], st[k]);
        }
        fy_result_stats(res, &stats);
        fy_result_itemcf_estimate_stats(res, &estimateStats);
        return res;
    }

    // "Because you liked ...": Mahout's ItemBasedRecommender.recommendedBecause asked of the distributed job
    // (fy_itemcf_because_prepared).  For every pair, in the order given, the kept preferences of the user whose similarity rows hold the
    // item -- the terms of the sum estimatePairs finishes -- the howMany (1 .. FY_BECAUSE_MAX) heaviest listed: weight pref * sim
    // descending, equal weights by ascending item id, NaN last.  estimate / status are estimatePairs' bit for bit; contributors counts
    // all terms, listed or not.  The rows of pair t are start[t] .. start[t + 1].
    struct Explanations {
        std::vector<int32_t> user, item, status, contributors;      // per pair
        std::vector<float> estimate;
        std::vector<int64_t> start;                                 // pairs + 1
        std::vector<int32_t> pair, because;                         // per row
        std::vector<float> sim, pref;
    };
    fy_itemcf_because_stats becauseStats{};
    Explanations recommendedBecause(PreparedItemSimilarity& prepared, const std::vector<int32_t>& users, const std::vector<int32_t>& items,
                                    int32_t howMany, int32_t maxPrefs, bool boolean) {
        if (!prepared.job()) throw std::runtime_error("BaselineRecommenderJob failed!: recommendedBecause on a closed prepared job");
        if (users.size() != items.size()) throw std::invalid_argument("recommendedBecause: users and items differ in length");
        fy_itemcf_params cp{};
        cp.max_prefs_per_user = maxPrefs;
        cp.boolean_data = boolean ? 1 : 0;
        cp.world = 1;
        fy_itemcf_pairs q{};
        q.n_pairs = (int64_t)users.size();
        q.users = users.empty() ? nullptr : users.data();
        q.items = items.empty() ? nullptr : items.data();
        q.location = FY_HOST;
        fy_result* res = nullptr;
        if (fy_itemcf_because_prepared(prepared.job(), &cp, &q, howMany, &res) != FY_OK)
            throw std::runtime_error(std::string("BaselineRecommenderJob failed!: because: ") + fy_last_error());
        fy_itemcf_because_view v{};
        if (fy_result_because_view(res, &v) != FY_OK) {
            fy_result_free(res);
            throw std::runtime_error(std::string("BaselineRecommenderJob failed!: because: ") + fy_last_error());
        }
        Explanations e;
        const int64_t np = v.n_pairs, n = fy_result_size(res);
        e.user.assign(v.user, v.user + np);
        e.item.assign(v.item, v.item + np);
        e.status.assign(v.status, v.status + np);
        e.contributors.assign(v.contributors, v.contributors + np);
        e.estimate.assign(v.estimate, v.estimate + np);
        e.start.assign(v.start, v.start + np + 1);
        const int32_t *pair = fy_result_aux(res), *because = fy_result_key1(res);
        const float* sim = fy_result_value(res);
        e.pair.assign(pair, pair + n);
        e.because.assign(because, because + n);
        e.sim.assign(sim, sim + n);
        e.pref.assign(v.pref, v.pref + n);
        fy_result_stats(res, &stats);
        fy_result_itemcf_because_stats(res, &becauseStats);
        fy_result_free(res);
        return e;
    }
};

// Fold-in of given profiles on standing factors (fy_foldin_*; include/filmyou.h): the cluster of a visitor nobody has seen, from the item
// factors W of the last PPC / NMF run, without a factorisation and without a prepare.  Owns its context and model (move-only).  Only
// whole profiles are taken: a resident row with pending writes is composed by the caller.
class FoldIn {
   public:
    using Profiles = BaselineRecommenderJob::Profiles;      // label, start, item, score, remove
    struct Assignment {
        std::vector<int32_t> label, cluster, parent, status;      // status: FY_FOLDIN_*
        std::vector<double> factors;                                // profiles x k, the top-level rows
        std::vector<int64_t> subOffset;                             // profiles + 1 into subFactors
        std::vector<double> subFactors;                             // the second-level rows, ragged
        fy_foldin_stats stats{};
    };

    // W: numberOfItems x k, row r = item id r + 1; counts: a `clusteringCount` (empty = every column may win)
    FoldIn(const std::vector<double>& W, int32_t numberOfItems, int32_t k, bool ppc = true, int32_t normalizationFrequency = -1,
           const std::vector<int32_t>& counts = {}, int device = 0) : k_(k) {
        if ((int64_t)W.size() != (int64_t)numberOfItems * k) throw std::invalid_argument("W must hold numberOfItems x k values");
        if (fy_context_create(device, &ctx_) != FY_OK) throw std::runtime_error(std::string("FoldIn failed!: ") + fy_last_error());
        const fy_foldin_params p{numberOfItems, k, ppc ? 1 : 0, normalizationFrequency};
        if (fy_foldin_create(ctx_, &p, W.data(), FY_HOST, counts.empty() ? nullptr : counts.data(), (int64_t)counts.size(), &model_) != FY_OK) {
            const std::string msg = fy_last_error();
            close();
            throw std::runtime_error("FoldIn failed!: " + msg);
        }
    }
    FoldIn(const FoldIn&) = delete;
    FoldIn& operator=(const FoldIn&) = delete;
    FoldIn(FoldIn&& o) noexcept : ctx_(o.ctx_), model_(o.model_), k_(o.k_) { o.ctx_ = nullptr; o.model_ = nullptr; }
    ~FoldIn() { close(); }

    // the refined level: per parent its item count, sub-cluster count, ascending raw item ids and W_c, in the layout of
    // fy_submap_items / fy_refined_factors; counts: the refined `clusteringCount`
    void addLevel(const std::vector<int32_t>& itemsInCluster, const std::vector<int32_t>& subClusters, const std::vector<int32_t>& itemRaw,
                  const std::vector<double>& Wragged, int32_t stride, const std::vector<int32_t>& counts = {}) {
        if (itemsInCluster.size() != subClusters.size()) throw std::invalid_argument("itemsInCluster and subClusters differ in length");
        if (fy_foldin_add_level(model_, (int32_t)subClusters.size(), itemsInCluster.data(), subClusters.data(), itemRaw.data(), Wragged.data(), stride,
                                counts.empty() ? nullptr : counts.data(), (int64_t)counts.size()) != FY_OK)
            throw std::runtime_error(std::string("FoldIn failed!: ") + fy_last_error());
    }

    // h0: profiles x k starting rows (top level) or empty = uniform 1 / k
    Assignment assign(const Profiles& profiles, int32_t iterations = 10, int32_t firstIteration = 1, const std::vector<double>& h0 = {}, int32_t rank = 0,
                      int32_t world = 1) {
        if (!h0.empty() && h0.size() != profiles.label.size() * (size_t)k_) throw std::invalid_argument("h0 must hold profiles x k values");
        const fy_itemcf_profiles q{(int64_t)profiles.label.size(), profiles.label.data(), profiles.start.data(), profiles.item.data(), profiles.score.data(),
                                   profiles.remove.data(), FY_PROFILE_WHOLE};
        fy_foldin_result* res = nullptr;
        if (fy_foldin_assign(model_, &q, iterations, firstIteration, h0.empty() ? nullptr : h0.data(), rank, world, &res) != FY_OK)
            throw std::runtime_error(std::string("FoldIn failed!: ") + fy_last_error());
        Assignment a;
        const size_t n = (size_t)fy_foldin_result_n(res);
        a.label.resize(n); a.cluster.resize(n); a.parent.resize(n); a.status.resize(n);
        a.factors.resize(n * (size_t)k_);
        a.subOffset.resize(n + 1);
        a.subFactors.resize((size_t)fy_foldin_result_sub_size(res));
        int rc = fy_foldin_result_assignment(res, a.label.data(), a.cluster.data(), a.parent.data(), a.status.data());
        if (rc == FY_OK) rc = fy_foldin_result_factors(res, a.factors.data());
        if (rc == FY_OK) rc = fy_foldin_result_sub_factors(res, a.subOffset.data(), a.subFactors.data());
        if (rc == FY_OK) rc = fy_foldin_result_stats(res, &a.stats);
        fy_foldin_result_free(res);
        if (rc != FY_OK) throw std::runtime_error(std::string("FoldIn failed!: ") + fy_last_error());
        return a;
    }
    int32_t k() const { return k_; }
    void close() {
        if (model_) fy_foldin_destroy(model_);
        if (ctx_) fy_context_destroy(ctx_);
        model_ = nullptr;
        ctx_ = nullptr;
    }

   private:
    fy_context* ctx_ = nullptr;
    fy_foldin* model_ = nullptr;
    int32_t k_ = 0;
};

}  // namespace host
}  // namespace fy
