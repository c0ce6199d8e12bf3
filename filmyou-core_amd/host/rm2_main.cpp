// rm2_main.cpp -- a tiny C++ driver over fy::host::RM2Job, used by tests/test_cpp_host_gpu.py.
//   rm2_main <ratings.txt> <clustering.txt|-> <lambda> <numberOfItems> <numberOfClusters> <numberOfRecommendations>
// ratings.txt: "user item score" per line; clustering.txt: "user cluster" per line.  Prints "user item score cluster".
// Trailing key=value arguments (smoothing=dirichlet mu=100) are put into the job's Configuration as they are.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "filmyou_job.hpp"

// rm2_main --files <mapred.input.dir> <mapred.output.dir> <directory> <lambda> <numberOfItems> <numberOfClusters> <numberOfRecommendations>
//   : RM2Job::runFiles on the reference's SequenceFile layout.
// rm2_main --rccl <ratings.txt> <clustering.txt|-> <lambda> <numberOfItems> <numberOfClusters> <numberOfRecommendations>
//   : RM2Job::runRank as rank 0 of a world of 1 through the compiled RCCL transport (fy_rccl_*).
static int main_files(char** a) {
    fy::host::Configuration conf;
    conf.set("mapred.input.dir", a[0]); conf.set("mapred.output.dir", a[1]); conf.set("directory", a[2]);
    conf.set("lambda", a[3]); conf.set("numberOfItems", a[4]); conf.set("numberOfClusters", a[5]); conf.set("numberOfRecommendations", a[6]);
    try {
        fy::host::RM2Job job(conf);
        job.runFiles();
        fprintf(stderr, "totalSum %.17g recs %lld\n", job.totalSum, (long long)job.stats.recs);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

// rm2_main --similar-items <items.txt> <ratings.txt> <similarityClassname> <K>
//   : RowSimilarityJob::runItems, the similarity rows of the ids of the items file alone.  Prints "item other sim".
static int main_similar_items(char** a) {
    fy::host::Ratings r;
    FILE* f = fopen(a[1], "r");
    if (!f) { perror(a[1]); return 2; }
    int u, i; float s;
    while (fscanf(f, "%d %d %f", &u, &i, &s) == 3) r.add(u, i, s);
    fclose(f);
    int64_t n = 0;
    int32_t* ids = nullptr;
    if (fy_idfile_read(a[0], &n, &ids) != FY_OK) { fprintf(stderr, "RowSimilarityJob failed!: %s\n", fy_last_error()); return 1; }
    std::vector<int32_t> items(ids, ids + n);
    fy_buffer_free(ids);
    try {
        fy::host::RowSimilarityJob job;
        job.runItems(r, items, a[2], atoi(a[3]), true, nullptr, [](int32_t item, int32_t other, float sim) { printf("%d %d %.9g\n", item, other, sim); });
        fprintf(stderr, "request items_known %lld rows_emitted %lld batches %lld pair_contribs %lld\n", (long long)job.requestStats.items_known,
                (long long)job.requestStats.rows_emitted, (long long)job.requestStats.batches, (long long)job.requestStats.pair_contribs);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

// rm2_main --recommend-users <users.txt> <ratings.txt> <similarityClassname> <K> <N> <maxPrefs>
//   : BaselineRecommenderJob::prepare + recommendUsers, item-based lists for the ids of the users file alone.  Prints "user item score".
static int main_recommend_users(char** a) {
    fy::host::Ratings r;
    FILE* f = fopen(a[1], "r");
    if (!f) { perror(a[1]); return 2; }
    int u, i; float s;
    while (fscanf(f, "%d %d %f", &u, &i, &s) == 3) r.add(u, i, s);
    fclose(f);
    int64_t n = 0;
    int32_t* ids = nullptr;
    if (fy_idfile_read(a[0], &n, &ids) != FY_OK) { fprintf(stderr, "BaselineRecommenderJob failed!: %s\n", fy_last_error()); return 1; }
    std::vector<int32_t> users(ids, ids + n);
    fy_buffer_free(ids);
    try {
        fy::host::BaselineRecommenderJob job;
        job.similarityClassname = a[2];
        job.maxSimilaritiesPerItem = atoi(a[3]);
        job.numRecommendations = atoi(a[4]);
        job.maxPrefsPerUser = atoi(a[5]);
        fy::host::PreparedItemSimilarity prepared = job.prepare(r);
        job.recommendUsers(prepared, users, [](int32_t user, int32_t item, float score) { printf("%d %d %.9g\n", user, item, score); });
        const fy_itemcf_request_stats& q = job.requestStats;
        fprintf(stderr, "request users_known %lld items_needed %lld rows_built %lld rows_from_store %lld rows_stored %lld batches %lld pair_contribs %lld\n",
                (long long)q.users_known, (long long)q.items_needed, (long long)q.rows_built, (long long)q.rows_from_store, (long long)q.rows_stored,
                (long long)q.batches, (long long)q.pair_contribs);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

// rm2_main --recommend-profiles <profiles.txt> --profile-base whole|resident <ratings.txt> <similarityClassname> <K> <N> <maxPrefs>
//   : BaselineRecommenderJob::prepare on the ratings + recommendProfiles.  <profiles.txt>: "label item score" per line, in the style of
//   the --estimate-pairs file; consecutive lines with one label form one profile (the same label again later begins another), their
//   order is the order of the entries.  A score of "x" is the delete marker: "label item x" deletes the item from the profile.
//   whole: each profile is a whole preference vector; resident: it is applied on top of the prepared row of user <label>.
//   Prints "label item score" as --recommend-users does; one `profiles ...` line of counters on stderr.
static int main_recommend_profiles(char** a) {
    const char* base = a[2];
    if (strcmp(a[1], "--profile-base") != 0 || (strcmp(base, "whole") != 0 && strcmp(base, "resident") != 0)) {
        fprintf(stderr, "usage: --recommend-profiles FILE --profile-base whole|resident ratings similarityClassname K N maxPrefs\n"
                        "  FILE: 'label item score' per line, consecutive lines with one label form one profile; 'label item x' deletes the item\n");
        return 2;
    }
    fy::host::Ratings r;
    FILE* f = fopen(a[3], "r");
    if (!f) { perror(a[3]); return 2; }
    int u, i; float s;
    while (fscanf(f, "%d %d %f", &u, &i, &s) == 3) r.add(u, i, s);
    fclose(f);
    fy::host::BaselineRecommenderJob::Profiles profiles;
    profiles.resident = strcmp(base, "resident") == 0;
    f = fopen(a[0], "r");
    if (!f) { perror(a[0]); return 2; }
    char word[64];
    bool any = false;
    int last = 0;
    while (fscanf(f, "%d %d %63s", &u, &i, word) == 3) {
        if (!any || u != last) profiles.begin(u);
        any = true;
        last = u;
        if (strcmp(word, "x") == 0) profiles.del(i); else profiles.put(i, strtof(word, nullptr));
    }
    fclose(f);
    try {
        fy::host::BaselineRecommenderJob job;
        job.similarityClassname = a[4];
        job.maxSimilaritiesPerItem = atoi(a[5]);
        job.numRecommendations = atoi(a[6]);
        job.maxPrefsPerUser = atoi(a[7]);
        fy::host::PreparedItemSimilarity prepared = job.prepare(r);
        job.recommendProfiles(prepared, profiles, [](int32_t user, int32_t item, float score) { printf("%d %d %.9g\n", user, item, score); });
        const fy_itemcf_profile_stats& q = job.profileStats;
        fprintf(stderr, "profiles asked %lld scored %lld empty %lld users_unknown %lld entries %lld unknown_item %lld superseded %lld removes_hit %lld "
                "removes_missed %lld prefs_composed %lld items_needed %lld rows_built %lld\n", (long long)q.profiles_asked, (long long)q.profiles_scored,
                (long long)q.profiles_empty, (long long)q.users_unknown, (long long)q.entries, (long long)q.entries_unknown_item,
                (long long)q.entries_superseded, (long long)q.removes_hit, (long long)q.removes_missed, (long long)q.prefs_composed,
                (long long)q.items_needed, (long long)q.rows_built);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

// rm2_main --fold-in <profiles.txt> <W.txt> <k> <iterations> <ppc> <normalizationFrequency>
//   : FoldIn::assign, the cluster of every profile from the standing item factors.  <profiles.txt> in the format of --recommend-profiles;
//   <W.txt>: one row of k values per line, row r = item id r + 1.  Prints "label cluster status" followed by the k values of the
//   profile's factor row (%.17g); one `foldin ...` line of counters on stderr.
static int main_fold_in(char** a) {
    const int k = atoi(a[2]);
    if (k <= 0) { fprintf(stderr, "usage: --fold-in PROFILES W.txt k iterations ppc normalizationFrequency\n"); return 2; }
    std::vector<double> W;
    FILE* f = fopen(a[1], "r");
    if (!f) { perror(a[1]); return 2; }
    double v;
    while (fscanf(f, "%lf", &v) == 1) W.push_back(v);
    fclose(f);
    if (W.empty() || W.size() % (size_t)k != 0) { fprintf(stderr, "%s: %zu values are not rows of %d\n", a[1], W.size(), k); return 2; }
    fy::host::FoldIn::Profiles profiles;
    f = fopen(a[0], "r");
    if (!f) { perror(a[0]); return 2; }
    char word[64];
    bool any = false;
    int u, i, last = 0;
    while (fscanf(f, "%d %d %63s", &u, &i, word) == 3) {
        if (!any || u != last) profiles.begin(u);
        any = true;
        last = u;
        if (strcmp(word, "x") == 0) profiles.del(i); else profiles.put(i, strtof(word, nullptr));
    }
    fclose(f);
    try {
        fy::host::FoldIn fold(W, (int32_t)(W.size() / (size_t)k), k, atoi(a[4]) != 0, atoi(a[5]));
        const fy::host::FoldIn::Assignment r = fold.assign(profiles, atoi(a[3]));
        for (size_t p = 0; p < r.label.size(); p++) {
            printf("%d %d %d", r.label[p], r.cluster[p], r.status[p]);
            for (int c = 0; c < k; c++) printf(" %.17g", r.factors[p * (size_t)k + c]);
            printf("\n");
        }
        const fy_foldin_stats& q = r.stats;
        fprintf(stderr, "foldin asked %lld assigned %lld empty %lld no_cluster %lld entries %lld out_of_range %lld superseded %lld removed %lld "
                "nonpositive %lld items_composed %lld launches %lld\n", (long long)q.profiles_asked, (long long)q.profiles_assigned, (long long)q.profiles_empty,
                (long long)q.profiles_no_cluster, (long long)q.entries, (long long)q.entries_out_of_range, (long long)q.entries_superseded,
                (long long)q.entries_removed, (long long)q.entries_nonpositive, (long long)q.items_composed, (long long)q.launches);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

// rm2_main --estimate-pairs <test.txt> <ratings.txt> <similarityClassname> <K> <maxPrefs>
//   : BaselineRecommenderJob::prepare on the ratings + estimatePairs for the (user, item) of the test ratings ("user item score" per line)
//   + estimateErrors against their scores.  <test.txt> = holdout:<fraction>:<seed> splits <ratings.txt> instead: prepared on the train side.
//   Prints "user item estimate status"; one `estimate ...` line on stderr.
static int main_estimate_pairs(char** a) {
    fy::host::Ratings r, test;
    FILE* f = fopen(a[1], "r");
    if (!f) { perror(a[1]); return 2; }
    int u, i; float s;
    while (fscanf(f, "%d %d %f", &u, &i, &s) == 3) r.add(u, i, s);
    fclose(f);
    try {
        double fraction = 0.0;
        unsigned long long seed = 0;
        if (sscanf(a[0], "holdout:%lf:%llu", &fraction, &seed) == 2) {
            auto parts = fy::host::holdout(r, fraction, seed);
            r = std::move(parts.first);
            test = std::move(parts.second);
            fprintf(stderr, "holdout train %zu test %zu\n", r.user.size(), test.user.size());
        } else {
            f = fopen(a[0], "r");
            if (!f) { perror(a[0]); return 2; }
            while (fscanf(f, "%d %d %f", &u, &i, &s) == 3) test.add(u, i, s);
            fclose(f);
        }
        fy::host::BaselineRecommenderJob job;
        job.similarityClassname = a[2];
        job.maxSimilaritiesPerItem = atoi(a[3]);
        job.maxPrefsPerUser = atoi(a[4]);
        fy::host::PreparedItemSimilarity prepared = job.prepare(r);
        fy_result* est = job.estimatePairs(prepared, test.user, test.item,
                                           [](int32_t user, int32_t item, float v, int32_t status) { printf("%d %d %.9g %d\n", user, item, v, status); });
        fy_eval_errors e{};
        try {
            e = fy::host::estimateErrors(prepared.context(), est, test);
        } catch (...) {
            fy_result_free(est);
            throw;
        }
        fy_result_free(est);
        fprintf(stderr, "estimate pairs %lld estimated %lld truth_not_finite %lld ok %lld unknown_user %lld unknown_item %lld own_preference %lld too_few %lld "
                "zero_numerator %lld not_a_number %lld row_entries_walked %lld mae %.17g rmse %.17g\n", (long long)e.pairs, (long long)e.estimated,
                (long long)e.truth_not_finite, (long long)e.by_status[0], (long long)e.by_status[1], (long long)e.by_status[2], (long long)e.by_status[3],
                (long long)e.by_status[4], (long long)e.by_status[5], (long long)e.by_status[6], (long long)job.estimateStats.row_entries_walked,
                fy::host::mae(e), fy::host::rmse(e));
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

// rm2_main --because <pairs.txt> <ratings.txt> <similarityClassname> <K> <maxPrefs> <howMany>
//   : BaselineRecommenderJob::prepare on the ratings + recommendedBecause for the pairs ("user item" per line).
//   Prints "pair user item because sim pref" per listed row, then "# pair user item estimate status contributors" per pair; one
//   `because ...` line of counters on stderr.
static int main_because(char** a) {
    fy::host::Ratings r;
    std::vector<int32_t> users, items;
    FILE* f = fopen(a[1], "r");
    if (!f) { perror(a[1]); return 2; }
    int u, i; float s;
    while (fscanf(f, "%d %d %f", &u, &i, &s) == 3) r.add(u, i, s);
    fclose(f);
    f = fopen(a[0], "r");
    if (!f) { perror(a[0]); return 2; }
    while (fscanf(f, "%d %d", &u, &i) == 2) { users.push_back(u); items.push_back(i); }
    fclose(f);
    try {
        fy::host::BaselineRecommenderJob job;
        job.similarityClassname = a[2];
        job.maxSimilaritiesPerItem = atoi(a[3]);
        fy::host::PreparedItemSimilarity prepared = job.prepare(r);
        const auto e = job.recommendedBecause(prepared, users, items, atoi(a[5]), atoi(a[4]), false);
        for (size_t k = 0; k < e.pair.size(); k++) {
            const int32_t t = e.pair[k];
            printf("%d %d %d %d %.9g %.9g\n", t, e.user[t], e.item[t], e.because[k], e.sim[k], e.pref[k]);
        }
        for (size_t t = 0; t < e.user.size(); t++) printf("# %zu %d %d %.9g %d %d\n", t, e.user[t], e.item[t], e.estimate[t], e.status[t], e.contributors[t]);
        const fy_itemcf_because_stats& b = job.becauseStats;
        fprintf(stderr, "because pairs %lld rows %lld contributors %lld ok %lld unknown_user %lld unknown_item %lld own_preference %lld too_few %lld "
                "zero_numerator %lld not_a_number %lld users_known %lld targets %lld rows_built %lld row_entries_walked %lld\n", (long long)b.pairs_asked,
                (long long)b.rows, (long long)b.contributors, (long long)b.by_status[0], (long long)b.by_status[1], (long long)b.by_status[2],
                (long long)b.by_status[3], (long long)b.by_status[4], (long long)b.by_status[5], (long long)b.by_status[6], (long long)b.users_known,
                (long long)b.targets, (long long)b.rows_built, (long long)b.row_entries_walked);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    std::vector<std::pair<std::string, std::string>> extra;      // trailing key=value arguments
    while (argc > 1 && argv[argc - 1][0] != '-' && strchr(argv[argc - 1], '=') && !strchr(argv[argc - 1], '/')) {
        const char* eq = strchr(argv[argc - 1], '=');
        extra.emplace_back(std::string((const char*)argv[argc - 1], (size_t)(eq - argv[argc - 1])), std::string(eq + 1));
        argc--;
    }
    if (argc == 9 && strcmp(argv[1], "--files") == 0) return main_files(argv + 2);
    if (argc == 8 && strcmp(argv[1], "--recommend-users") == 0) return main_recommend_users(argv + 2);
    if (argc == 10 && strcmp(argv[1], "--recommend-profiles") == 0) return main_recommend_profiles(argv + 2);
    if (argc == 6 && strcmp(argv[1], "--similar-items") == 0) return main_similar_items(argv + 2);
    if (argc == 7 && strcmp(argv[1], "--estimate-pairs") == 0) return main_estimate_pairs(argv + 2);
    if (argc == 8 && strcmp(argv[1], "--fold-in") == 0) return main_fold_in(argv + 2);
    if (argc == 8 && strcmp(argv[1], "--because") == 0) return main_because(argv + 2);
    // rm2_main --score-profiles <profiles.txt> --profile-base whole|resident [--profile-cluster C] <ratings.txt> ... : RM2Job::scoreProfiles.
    //   <profiles.txt> in the format of --recommend-profiles: "label item score" per line, consecutive lines with one label form one
    //   profile, "label item x" deletes the item.  whole: every profile is scored in cluster C (default 0) as one more member of it;
    //   resident: the entries go on top of the prepared row of user <label>.  One `profiles ...` line of counters on stderr.
    const char* profiles_file = nullptr;
    const char* profile_base = nullptr;
    int profile_cluster = 0;
    if (argc >= 11 && strcmp(argv[1], "--score-profiles") == 0 && strcmp(argv[3], "--profile-base") == 0) {
        profiles_file = argv[2];
        profile_base = argv[4];
        argv += 4; argc -= 4;
        if (argc == 9 && strcmp(argv[1], "--profile-cluster") == 0) { profile_cluster = atoi(argv[2]); argv += 2; argc -= 2; }
        if (argc != 7 || (strcmp(profile_base, "whole") != 0 && strcmp(profile_base, "resident") != 0)) {
            fprintf(stderr, "usage: --score-profiles FILE --profile-base whole|resident [--profile-cluster C] ratings clustering lambda numberOfItems "
                            "numberOfClusters numberOfRecommendations\n");
            return 2;
        }
    }
    bool rccl = false;
    // rm2_main --users <users.txt> <ratings.txt> ... : RM2Job::runUsers, lists for the ids of the usersFile alone
    const char* users_file = nullptr;
    if (argc == 9 && !profiles_file && strcmp(argv[1], "--users") == 0) { users_file = argv[2]; argv += 2; argc -= 2; }
    if (argc == 8 && strcmp(argv[1], "--rccl") == 0) { rccl = true; argv++; argc--; }
    // rm2_main --writes <writes.txt> <ratings.txt> ... : fy::host::applyWrites first ("user item score remove" per line, in order), the job on the result
    const char* writes_file = nullptr;
    if (argc == 9 && !users_file && strcmp(argv[1], "--writes") == 0) { writes_file = argv[2]; argv += 2; argc -= 2; }
    // rm2_main --evaluate <test.txt> <cutoff> <ratings.txt> ... : RM2Job::runEvaluated, the job's lists evaluated on the GPU against the test
    // ratings ("user item score" per line) at that cutoff; relevanceThreshold=<x> (default 4) may trail.  One `eval ...` line on stderr.
    // <test.txt> = holdout:<fraction>:<seed> splits <ratings.txt> instead (fy::host::holdout): the job runs on the train side.
    const char* eval_file = nullptr;
    int eval_cutoff = 0;
    if (argc == 10 && !users_file && !writes_file && strcmp(argv[1], "--evaluate") == 0) { eval_file = argv[2]; eval_cutoff = atoi(argv[3]); argv += 3; argc -= 3; }
    if (argc != 7) { fprintf(stderr, "usage: %s ratings clustering lambda numberOfItems numberOfClusters numberOfRecommendations\n", argv[0]); return 2; }
    fy::host::Ratings r;
    fy::host::Clustering c;
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int u, i; float s;
    while (fscanf(f, "%d %d %f", &u, &i, &s) == 3) r.add(u, i, s);
    fclose(f);
    if (strcmp(argv[2], "-") != 0) {
        f = fopen(argv[2], "r");
        if (!f) { perror(argv[2]); return 2; }
        int cl;
        while (fscanf(f, "%d %d", &u, &cl) == 2) { c.user.push_back(u); c.cluster.push_back(cl); }
        fclose(f);
    }
    fy::host::Configuration conf;
    conf.set("lambda", argv[3]);
    conf.set("numberOfItems", argv[4]);
    conf.set("numberOfClusters", argv[5]);
    conf.set("numberOfRecommendations", argv[6]);
    for (const auto& kv : extra) conf.set(kv.first, kv.second);
    try {
        if (writes_file) {
            fy::host::Writes w;
            f = fopen(writes_file, "r");
            if (!f) { perror(writes_file); return 2; }
            int gone;
            while (fscanf(f, "%d %d %f %d", &u, &i, &s, &gone) == 4) { if (gone) w.del(u, i); else w.put(u, i, s); }
            fclose(f);
            fy_ratings_update_stats us{};
            r = fy::host::applyWrites(r, w, &us);
            fprintf(stderr, "writes %lld superseded %lld replaced %lld inserted %lld deleted %lld delete_missed %lld source_dropped %lld nnz_out %lld\n",
                    (long long)us.n_writes, (long long)us.n_superseded, (long long)us.n_replaced, (long long)us.n_inserted, (long long)us.n_deleted,
                    (long long)us.n_delete_missed, (long long)us.n_source_dropped, (long long)us.nnz_out);
        }
        if (users_file) conf.set("usersFile", users_file);      // (the job copies its configuration)
        fy::host::RM2Job job(conf);
        auto sink = [](int32_t user, int32_t item, float score, int32_t cluster) { printf("%d %d %.9g %d\n", user, item, score, cluster); };
        if (profiles_file) {
            fy::host::RM2Job::Profiles profiles;
            profiles.resident = strcmp(profile_base, "resident") == 0;
            f = fopen(profiles_file, "r");
            if (!f) { perror(profiles_file); return 2; }
            char word[64];
            bool any = false;
            int last = 0;
            while (fscanf(f, "%d %d %63s", &u, &i, word) == 3) {
                if (!any || u != last) profiles.begin(u, profile_cluster);
                any = true;
                last = u;
                if (strcmp(word, "x") == 0) profiles.del(i); else profiles.put(i, strtof(word, nullptr));
            }
            fclose(f);
            job.scoreProfiles(r, c, profiles, sink);
            const fy_rm2_profile_stats& q = job.profileStats;
            fprintf(stderr, "profiles asked %lld scored %lld empty %lld users_unknown %lld users_filtered %lld entries %lld unknown_item %lld nonpositive %lld "
                    "superseded %lld removes_hit %lld removes_missed %lld items_composed %lld clusters_touched %lld slab_rows %lld\n",
                    (long long)q.profiles_asked, (long long)q.profiles_scored, (long long)q.profiles_empty, (long long)q.users_unknown,
                    (long long)q.users_filtered, (long long)q.entries, (long long)q.entries_unknown_item, (long long)q.entries_nonpositive,
                    (long long)q.entries_superseded, (long long)q.removes_hit, (long long)q.removes_missed, (long long)q.items_composed,
                    (long long)q.clusters_touched, (long long)q.slab_rows);
        } else if (users_file) {
            job.runUsers(r, c, {}, sink);
            fprintf(stderr, "request users_known %lld clusters_touched %lld slab_rows %lld full_pass_clusters %lld\n", (long long)job.requestStats.users_known,
                    (long long)job.requestStats.clusters_touched, (long long)job.requestStats.slab_rows, (long long)job.requestStats.full_pass_clusters);
        } else if (eval_file) {
            fy::host::Ratings test;
            double fraction = 0.0;
            unsigned long long seed = 0;
            if (sscanf(eval_file, "holdout:%lf:%llu", &fraction, &seed) == 2) {      // no file: the job runs on the train side of the split
                auto parts = fy::host::holdout(r, fraction, seed);
                r = std::move(parts.first);
                test = std::move(parts.second);
                fprintf(stderr, "holdout train %zu test %zu\n", r.user.size(), test.user.size());
            } else {
                f = fopen(eval_file, "r");
                if (!f) { perror(eval_file); return 2; }
                while (fscanf(f, "%d %d %f", &u, &i, &s) == 3) test.add(u, i, s);
                fclose(f);
            }
            job.runEvaluated(r, c, test, {eval_cutoff}, conf.getDouble("relevanceThreshold", 4.0), sink);
            const fy_eval_sums& e = job.evaluation;
            using E = fy::host::Evaluator;
            fprintf(stderr, "eval lists %lld users_evaluated %lld lists_without_relevant %lld relevant_users %lld relevant_entries %lld cutoff %d hits %lld users_hit %lld "
                    "precision %.17g recall %.17g map %.17g mrr %.17g ndcg %.17g\n", (long long)e.lists, (long long)e.users_evaluated,
                    (long long)e.lists_without_relevant, (long long)e.relevant_users, (long long)e.relevant_entries, (int)e.cutoffs[0], (long long)e.hits[0],
                    (long long)e.users_hit[0], E::meanPrecision(e, 0), E::meanRecall(e, 0), E::meanAP(e, 0), E::meanRR(e, 0), E::meanNDCG(e, 0));
        } else if (rccl) {
            char id[128];
            if (fy_rccl_unique_id(id) != FY_OK) { fprintf(stderr, "RM2 failed!: %s\n", fy_last_error()); return 1; }
            job.runRank(r, c, sink, 0, 0, 1, id);
            fprintf(stderr, "rccl all_gathers %lld reduce_scatters %lld bytes %lld\n", (long long)job.allGathers, (long long)job.reduceScatters, (long long)job.collectiveBytes);
        } else {
            job.run(r, c, sink);
        }
        fprintf(stderr, "totalSum %.17g users %zu items %zu recs %lld\n", job.totalSum, job.userSum.size(), job.itemColl.size(), (long long)job.stats.recs);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
