// C entry point of the host NJ driver (include/vft_host.h).  Plain C++11, no HIP: links against libvft_hip.so.
#include "../../include/vft_host.h"

#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <type_traits>

#include "NJDriver.h"
#include "KnuthRng.h"
#include "MLLengths.h"
#include "GtrModel.h"
#include "AAModels.h"
#include "SeqMatrix.h"
#include "ReadTree.h"
#include "ReadTransition.h"
#include "StageLog.h"

// CRC-32 (the zlib polynomial) of the last join order this process produced, per chunk of joins: lets a caller that only asked
// for the tree (vft_nj_newick at a million sequences) compare the join order with a prefix of the reference's `Join` lines
static std::mutex gJoinCrcMutex;
static std::vector<uint32_t> gJoinCrc;
static int64_t gJoinCrcChunk = 10000, gJoinCrcJoins = 0;

static uint32_t crc32Bytes(const unsigned char *p, size_t n) {
    static uint32_t table[256];
    static bool ready = false;
    if (!ready) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        ready = true;
    }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

template<typename JOINS>
static void recordJoinCrc(const JOINS &js) {
    std::lock_guard<std::mutex> lock(gJoinCrcMutex);
    gJoinCrc.clear();
    gJoinCrcJoins = (int64_t) js.size();
    std::vector<int32_t> buf((size_t) gJoinCrcChunk * 3);
    for (size_t k0 = 0; k0 + (size_t) gJoinCrcChunk <= js.size(); k0 += (size_t) gJoinCrcChunk) {
        for (size_t k = 0; k < (size_t) gJoinCrcChunk; k++) {
            buf[3 * k] = (int32_t) js[k0 + k].i;
            buf[3 * k + 1] = (int32_t) js[k0 + k].j;
            buf[3 * k + 2] = (int32_t) js[k0 + k].newnode;
        }
        gJoinCrc.push_back(crc32Bytes((const unsigned char *) buf.data(), buf.size() * 4));
    }
    /* the joins behind the last complete chunk, as one shorter chunk (a finished run is compared to its last join) */
    const size_t done = js.size() / (size_t) gJoinCrcChunk * (size_t) gJoinCrcChunk;
    if (done < js.size()) {
        for (size_t k = 0; done + k < js.size(); k++) {
            buf[3 * k] = (int32_t) js[done + k].i;
            buf[3 * k + 1] = (int32_t) js[done + k].j;
            buf[3 * k + 2] = (int32_t) js[done + k].newnode;
        }
        gJoinCrc.push_back(crc32Bytes((const unsigned char *) buf.data(), (js.size() - done) * 3 * 4));
    }
}

extern "C" int vft_nj_last_join_crcs(int64_t *chunk, int64_t *nJoins, uint32_t *crcs, int64_t cap, int64_t *nCrcs) {
    std::lock_guard<std::mutex> lock(gJoinCrcMutex);
    if (chunk) *chunk = gJoinCrcChunk;
    if (nJoins) *nJoins = gJoinCrcJoins;
    if (nCrcs) *nCrcs = (int64_t) gJoinCrc.size();
    if (crcs)
        for (int64_t k = 0; k < cap && k < (int64_t) gJoinCrc.size(); k++) crcs[k] = gJoinCrc[(size_t) k];
    return VFT_OK;
}

/* wall-clock of the stages of the last vft_nj_newick / vft_nj_ml_newick of this process (vft_nj_last_stage_seconds) */
static double gStage[8];
static int64_t gLanes[4];
static int64_t gWalkDual[2];   /* SPR chains of the last tree: dual commands sent, continuations the walk server ran on its own (vft_nj_last_walk_dual) */
static int64_t gLaneExchange[2];   /* lanes across ranks of the last tree: all-gathers, bytes received (vft_nj_last_lane_exchange) */
static double gGamma[3];   /* `-gamma` of the last tree: Gamma(nCat) log-likelihood, alpha, length factor (vft_nj_last_gamma) */

/* treePartitioning (NJ.tcc:5540-5750) on a tree given as arrays: pure host code, no context (tests pin it to the reference's own
   partitions).  out[cap] receives the subtree roots in the reference's hand-out order. */
extern "C" int vft_tree_partitioning(int64_t nNodes, const int64_t *childIn, int64_t root, int32_t penalty, int32_t threads, int32_t window,
                                     int64_t *out, int64_t cap, int64_t *nOut, double *speedup) {
    if (nNodes < 4 || !childIn || root < 0 || root >= nNodes || penalty < 0 || threads < 1 || !nOut) return VFT_ERR_INVALID;
    if (threads > nNodes) threads = (int32_t) nNodes;   /* (more threads than nodes cannot change the partition) */
    /* the arrays come from the caller: every child id in range and every node the child of at most one parent - a tree, so the walk
       below ends and stays inside the arrays */
    std::vector<char> seen((size_t) nNodes, 0);
    for (int64_t i = 0; i < 3 * nNodes; i++) {
        const int64_t ch = childIn[i];
        if (ch < -1 || ch >= nNodes || ch == root) return VFT_ERR_INVALID;
        if (ch >= 0) {
            if (seen[(size_t) ch]) return VFT_ERR_INVALID;
            seen[(size_t) ch] = 1;
        }
    }
    std::vector<int64_t> child(childIn, childIn + 3 * nNodes), order;
    std::vector<std::pair<int64_t, int>> stack(1, std::make_pair(root, 0));
    while (!stack.empty()) {   /* post-order of the internal nodes, children in stored order */
        const int64_t v = stack.back().first;
        const int k = stack.back().second;
        if ((int64_t) stack.size() > nNodes) return VFT_ERR_INVALID;   /* (a cycle that does not pass through the root) */
        if (k < 3 && child[3 * v + k] >= 0) {
            stack.back().second++;
            stack.push_back(std::make_pair(child[3 * v + k], 0));
        } else {
            stack.pop_back();
            if (child[3 * v] >= 0) order.push_back(v);
        }
    }
    double sp = 0;
    const std::vector<int64_t> res = veryfasttree::MLLengths<float>::partitionTree(nNodes, child, root, order, penalty, threads, window > 0 ? window : 50, &sp);
    *nOut = (int64_t) res.size();
    if (speedup) *speedup = sp;
    for (int64_t k = 0; out && k < cap && k < (int64_t) res.size(); k++) out[k] = res[(size_t) k];
    return VFT_OK;
}

/* the exchange layout of the lanes across ranks (MLLengths::laneShare / laneRecord), for the CPU test that runs it over gloo:
   out[0] = per, out[1] = k0, out[2] = k1 for rank `rank` of `world`; out[3] = the record index of item `item` in the gathered buffer */
extern "C" int vft_nj_lane_share(int64_t nItems, int32_t world, int32_t rank, int64_t item, int64_t *out) {
    if (nItems < 0 || world < 1 || rank < 0 || rank >= world || !out) return VFT_ERR_INVALID;
    size_t per, k0, k1;
    veryfasttree::MLLengths<float>::laneShare((size_t) nItems, (size_t) world, (size_t) rank, per, k0, k1);
    out[0] = (int64_t) per;
    out[1] = (int64_t) k0;
    out[2] = (int64_t) k1;
    out[3] = per > 0 && item >= 0 ? (int64_t) veryfasttree::MLLengths<float>::laneRecord((size_t) item, per) : -1;
    return VFT_OK;
}

/* the layout of the out-profile blocks' exchange (NJDriver::outProfileBlock), for the CPU test that runs it over gloo:
   out[0] = owner rank of block `block` of `parts`, out[1] = its slot in that rank's share, out[2] = slots per share, out[3], out[4] = the
   block's entries [i0, i1) of a list of n */
extern "C" int vft_nj_out_profile_block(int32_t parts, int32_t world, int32_t block, int64_t n, int64_t *out) {
    if (parts < 1 || world < 1 || block < 0 || block >= parts || n < 0 || !out) return VFT_ERR_INVALID;
    veryfasttree::NJDriver<float>::outProfileBlock(parts, world, block, n, out[0], out[1], out[2], out[3], out[4]);
    return VFT_OK;
}

extern "C" int vft_nj_last_lane_exchange(int64_t *out) {
    if (!out) return VFT_ERR_INVALID;
    out[0] = gLaneExchange[0];
    out[1] = gLaneExchange[1];
    return VFT_OK;
}

extern "C" int vft_nj_last_walk_dual(int64_t *out) {
    if (!out) return VFT_ERR_INVALID;
    out[0] = gWalkDual[0];
    out[1] = gWalkDual[1];
    return VFT_OK;
}

extern "C" int vft_nj_last_gamma(double *out) {
    if (!out) return VFT_ERR_INVALID;
    for (int i = 0; i < 3; i++) out[i] = gGamma[i];
    return VFT_OK;
}

extern "C" int vft_nj_last_stage_seconds(double *seconds, int64_t *counts) {
    if (seconds)
        for (int i = 0; i < 8; i++) seconds[i] = gStage[i];
    if (counts)
        for (int i = 0; i < 4; i++) counts[i] = gLanes[i];
    return VFT_OK;
}

/* `-log` (vft_nj_set_log): the descriptor the next runs write the reference's log lines to; -1 = none.  Process state, like the
   other last-run records above. */
static int gLogFd = -1;

extern "C" int vft_nj_set_log(int32_t fd) {
    gLogFd = fd < 0 ? -1 : fd;
    return VFT_OK;
}

extern "C" int vft_nj_get_log() { return gLogFd; }

/* the log's first line: what it holds of the reference's log and what it leaves out (every comparison skips it) */
static const char kLogHeader[] =
        "# veryfasttree-amd log: the reference's stage trees, TreeLogLk, GTR, rate-category and Gamma lines, its clock lines and summary; "
        "not written: Command, version and option echo, Dist/N**2, Top hits, Max-lk operations, progress and warning texts, "
        "anything above the default verbosity\n";

/* the sink of a run, or none: logging is off, or this is not rank 0 of a communicator */
static std::unique_ptr<veryfasttree::StageLog> openLog(const vft_comm *comm) {
    std::unique_ptr<veryfasttree::StageLog> sink;
    if (gLogFd >= 0 && !(comm && comm->world > 1 && comm->rank > 0)) {
        sink.reset(new veryfasttree::StageLog(gLogFd));
        sink->text(kLogHeader);
    }
    return sink;
}

static veryfasttree::NJOptions toOptions(const vft_nj_options *o) {
    veryfasttree::NJOptions opt;
    if (o) {
        opt.fastest = o->fastest != 0;
        opt.tophitsMult = o->tophits_mult;
        opt.tophitsClose = o->tophits_close;
        opt.tophitsRefresh = o->tophits_refresh;
        opt.topvisibleMult = o->topvisible_mult;
        opt.staleOutLimit = o->stale_out_limit;
        opt.fResetOutProfile = o->f_reset_out_profile;
        opt.nResetOutProfile = o->n_reset_out_profile;
        opt.useTopHits2nd = o->use_tophits_2nd != 0;
        opt.tophits2Safety = o->tophits2_safety;
        opt.tophits2Mult = o->tophits2_mult;
        opt.tophits2Refresh = o->tophits2_refresh;
        opt.scoredist = o->scoredist != 0 || o->aa_model != 0;
        opt.aaModel = o->aa_model;
        opt.comm = o->comm;
        opt.threads = o->threads > 1 ? o->threads : 1;
        opt.gamma = o->gamma != 0;
        opt.outProfileParts = o->out_profile_parts >= 2 ? o->out_profile_parts : 0;
        opt.slow = o->slow != 0;
        opt.pseudoWeight = o->pseudo_weight;
        opt.mlAccuracy = o->ml_accuracy > 1 ? o->ml_accuracy : 1;
        opt.slowNNI = o->slow_nni != 0;
        opt.nniRounds = o->nni_rounds > 0 ? o->nni_rounds : 0;
        opt.mlNNIRounds = o->ml_nni_rounds > 0 ? o->ml_nni_rounds : 0;
        opt.sprLength = o->spr_length > 0 ? o->spr_length : 10;
        if (o->debug_flags & VFT_NJ_DEBUG_HOST_JOINS) opt.deviceJoins = false;
        if (o->debug_flags & VFT_NJ_DEBUG_HOST_LISTS) opt.deviceLists = false;
        if (o->debug_flags & VFT_NJ_DEBUG_HOST_RESET) opt.deviceReset = false;
        if (o->debug_flags & VFT_NJ_DEBUG_NO_WALK_SERVER) opt.walkServer = false;
        if (o->debug_flags & VFT_NJ_DEBUG_NO_WALK_DUAL) opt.walkDual = false;
        if (o->debug_flags & VFT_NJ_DEBUG_SEED_BY_SEED) opt.seedBatch = 1;
        if (o->debug_flags & VFT_NJ_DEBUG_LEVEL_LENGTHS) opt.parallelLengths = true;
        if (o->debug_flags & VFT_NJ_SHARD_LEAF_BLOCKS) opt.shardLeafBlocks = true;
    }
    return opt;
}

/* the description of duplicates vft_nj_newick takes (unique_first / aln_next) as the alignment row -> unique sequence map */
static std::vector<int64_t> alnToUnique(const int64_t *uniqueFirst, const int64_t *alnNext, int64_t nSeqs, int64_t nAll) {
    std::vector<int64_t> out((size_t) nAll, -1);
    for (int64_t u = 0; u < nSeqs; u++)
        for (int64_t k = uniqueFirst[u]; k != -1; k = alnNext[k]) {
            if (k < 0 || k >= nAll || out[(size_t) k] >= 0) throw std::invalid_argument("unique_first / aln_next do not describe the alignment's duplicates");
            out[(size_t) k] = u;
        }
    for (int64_t k = 0; k < nAll; k++)
        if (out[(size_t) k] < 0) throw std::invalid_argument("unique_first / aln_next leave an alignment row without a unique sequence");
    return out;
}

static std::vector<std::string> splitNames(const char *names, int64_t nAll) {
    std::vector<std::string> nm;
    nm.reserve((size_t) nAll);
    const char *p = names;
    for (int64_t k = 0; k < nAll; k++) {
        nm.push_back(std::string(p));
        p += nm.back().size() + 1;
    }
    return nm;
}

static veryfasttree::ReadTreeResult readTreeText(const char *text, int64_t nAll, const char *names, const int64_t *uniqueFirst,
                                                 const int64_t *alnNext, int64_t nSeqs) {
    if (!text || !names || !uniqueFirst || !alnNext || nSeqs < 1 || nAll < nSeqs) throw std::invalid_argument("vft_read_tree: bad arguments");
    const std::vector<std::string> nm = splitNames(names, nAll);
    return veryfasttree::ReadTree::parse(text, strlen(text), nm, alnToUnique(uniqueFirst, alnNext, nSeqs, nAll),
                                         std::vector<int64_t>(uniqueFirst, uniqueFirst + nSeqs));
}

/* the parse of `-intree` alone (host/ReadTree.h): pure host code, no context */
extern "C" int vft_read_tree(const char *text, int64_t nAll, const char *names, const int64_t *uniqueFirst, const int64_t *alnNext,
                             int64_t nSeqs, int64_t *parent, int64_t *child, int64_t *root, int64_t *nNodes, char *warnings,
                             int64_t warningsCap, char *err, int32_t errLen) {
    try {
        if (!parent || !child || !root || !nNodes) throw std::invalid_argument("vft_read_tree: bad arguments");
        const veryfasttree::ReadTreeResult r = readTreeText(text, nAll, names, uniqueFirst, alnNext, nSeqs);
        for (int64_t v = 0; v < 2 * nSeqs; v++) {
            parent[v] = v < r.nNodes ? r.parent[(size_t) v] : -1;
            for (int k = 0; k < 3; k++) child[3 * v + k] = v < r.nNodes ? r.child[(size_t) (3 * v + k)] : -1;
        }
        *root = r.root;
        *nNodes = r.nNodes;
        if (warnings && warningsCap > 0) {
            std::string w;
            for (const std::string &line: r.warnings) w += line + "\n";
            snprintf(warnings, (size_t) warningsCap, "%s", w.c_str());
        }
        return VFT_OK;
    } catch (const std::exception &e) {
        if (err && errLen > 0) snprintf(err, (size_t) errLen, "%s", e.what());
        return VFT_ERR_INVALID;
    }
}

/* `-intree`: what is not built is refused before anything reaches the device (include/vft_host.h, vft_nj_options.intree) */
static void checkIntree(const vft_nj_options *o, int64_t nSeqs) {
    if (!o || !o->intree) return;
    if (o->slow) throw std::invalid_argument("-intree with -slow is not built: the reference's NNI and SPR stages behave differently under -slow "
                                             "(NJ.tcc:1883-1901, 5980, 6267-6284), and the option's own stage, the exhaustive join search, does not run with a starting tree");
    if (o->comm && o->comm->world > 1) throw std::invalid_argument("-intree with a vft_comm of more than one rank is not built");
    if (nSeqs < 4) throw std::invalid_argument("-intree needs at least 4 unique sequences");
}

/* `-slow`: what is not built is refused before anything reaches the device (include/vft_host.h, vft_nj_options.slow) */
static void checkSlow(const vft_nj_options *o) {
    if (!o || !o->slow) return;
    if (o->fastest) throw std::invalid_argument("-slow and -fastest exclude each other (VeryFastTree.cpp:109-111)");
    if (o->me_nni || o->spr || o->ml_nni)
        throw std::invalid_argument("-slow with me_nni, spr or ml_nni is not built: the reference's NNI and SPR stages behave differently under "
                                    "-slow (NJ.tcc:1883-1901, 5980, 6267-6284); use -slow with -noml -nome or with -nome -mllen");
    if (o->comm && o->comm->world > 1) throw std::invalid_argument("-slow with a vft_comm of more than one rank is not built");
}

/* `-pseudo`: what is not built is refused before anything reaches the device (include/vft_host.h, vft_nj_options.pseudo_weight) */
static void checkPseudo(const vft_nj_options *o) {
    if (!o || o->pseudo_weight == 0) return;
    if (!(o->pseudo_weight > 0) || !std::isfinite(o->pseudo_weight)) throw std::invalid_argument("-pseudo takes a finite weight >= 0");
    if (o->comm && o->comm->world > 1)
        throw std::invalid_argument("-pseudo with a vft_comm of more than one rank is not built: the lane exchange of the subtree schedule carries "
                                    "six distances per quartet and no weights");
}

/* the thorough search (`-mlacc`, `-slownni`, `-nni`, `-mlnni`, `-sprlength`): refused before anything reaches the device, each message
   names its member (include/vft_host.h, vft_nj_options.ml_accuracy ... spr_length) */
static void checkThorough(const vft_nj_options *o) {
    if (!o) return;
    const struct {
        const char *name, *flag;
        int32_t value;
    } members[5] = {{"ml_accuracy", "-mlacc", o->ml_accuracy}, {"slow_nni", "-slownni", o->slow_nni}, {"nni_rounds", "-nni", o->nni_rounds},
                    {"ml_nni_rounds", "-mlnni", o->ml_nni_rounds}, {"spr_length", "-sprlength", o->spr_length}};
    for (const auto &m: members)
        if (m.value < 0)
            throw std::invalid_argument(std::string("vft_nj_options.") + m.name + " (" + m.flag + ") is negative: 0 is the reference's default");
    if (o->spr_length > 64)
        throw std::invalid_argument("vft_nj_options.spr_length (-sprlength) is above 64: the chain buffers of MLLengths::sprAttempt hold 64 steps");
}

/* `-trans`: the model "the matrix that was set" without one is refused before anything reaches the device - never a silent JTT run
   (include/vft_host.h, vft_nj_set_aa_transition) */
static void checkAAModel(const vft_nj_options *o) {
    if (!o || o->aa_model != veryfasttree::AA_MODEL_CUSTOM) return;
    if (!veryfasttree::customAATransition().set)
        throw std::invalid_argument("vft_nj_options.aa_model = 4 (-trans) without a matrix: vft_nj_set_aa_transition comes first");
}

/* the rounds of the refinement stages (host/NJDriver.h meNNIRoundsToDo / mlNNIRoundsToDo / sprBehindNNIRound), pure host code */
extern "C" int vft_nj_round_plan(int64_t nSeqs, int32_t nniRounds, int32_t mlNNIRounds, int32_t spr, int64_t *out, int64_t *sprBehind, int64_t cap) {
    if (nSeqs < 1 || nniRounds < 0 || mlNNIRounds < 0 || spr < 0 || !out) return VFT_ERR_INVALID;
    const int64_t nniToDo = veryfasttree::meNNIRoundsToDo(nSeqs, nniRounds), mlToDo = veryfasttree::mlNNIRoundsToDo(nSeqs, mlNNIRounds);
    out[0] = nniToDo;
    out[1] = mlToDo;
    out[2] = mlToDo - 2;
    int64_t k = 0;
    for (int64_t i = 0; i < nniToDo && k < spr; i++)
        if (veryfasttree::sprBehindNNIRound(i, nniToDo, spr)) {
            if (sprBehind && k < cap) sprBehind[k] = i + 1;
            k++;
        }
    for (; k < spr; k++)
        if (sprBehind && k < cap) sprBehind[k] = nniToDo;
    return VFT_OK;
}

extern "C" int vft_pseudo_distances(int32_t nProfiles, int32_t precision, const void *dist, const void *weight, double pseudoWeight, int32_t scoredist,
                                    double *out) {
    if ((nProfiles != 3 && nProfiles != 4) || (precision != 4 && precision != 8) || !dist || !weight || !out) return VFT_ERR_INVALID;
    if (!(pseudoWeight >= 0) || !std::isfinite(pseudoWeight)) return VFT_ERR_INVALID;
    const int nPairs = nProfiles * (nProfiles - 1) / 2;
    if (precision == 8) veryfasttree::pseudoDistances<double>(nPairs, (const double *) dist, (const double *) weight, pseudoWeight, scoredist != 0, out);
    else veryfasttree::pseudoDistances<float>(nPairs, (const float *) dist, (const float *) weight, pseudoWeight, scoredist != 0, out);
    return VFT_OK;
}

template<typename REAL>
static std::string runTree(vft_ctx *ctx, const uint8_t *codes, int64_t nSeqs, int64_t nPos, const vft_nj_options *o,
                           bool meLengths, int32_t nBootstrap, const int64_t *uniqueFirst, const int64_t *alnNext,
                           int64_t nAll, const char *names, std::vector<double> &loglk, std::vector<double> &rates,
                           std::vector<int64_t> &ratecat, double *gtrOut) {
    /* `-intree`: the text is parsed before anything reaches the device - a malformed tree costs no upload */
    veryfasttree::ReadTreeResult tree;
    if (o && o->intree) tree = readTreeText(o->intree, nAll, names, uniqueFirst, alnNext, nSeqs);
    /* the log opens behind every refusal - the option checks of the caller, the parse above: a run that is refused writes nothing */
    if (o && o->aa_model == veryfasttree::AA_MODEL_CUSTOM) {   /* VeryFastTree.cpp:100 */
        int32_t nCodes = 0;
        if (vft_get_n_codes(ctx, &nCodes) != VFT_OK || nCodes != 20) throw std::invalid_argument("-trans is an amino-acid model: the context holds nucleotides");
    }
    const std::unique_ptr<veryfasttree::StageLog> sink = openLog(o ? o->comm : nullptr);
    veryfasttree::StageLog *const log = sink.get();
    veryfasttree::NJDriver<REAL> drv(ctx, codes, nSeqs, nPos, toOptions(o));
    const std::vector<std::string> nm = splitNames(names, nAll);
    const std::vector<int64_t> uf(uniqueFirst, uniqueFirst + nSeqs), an(alnNext, alnNext + nAll);
    drv.setLog(log, &nm, &uf, &an);
    /* the rounds the reference announces (VeryFastTreeImpl.tcc:145-149) */
    const int64_t nniToDo = o && o->me_nni ? veryfasttree::meNNIRoundsToDo(nSeqs, o->nni_rounds > 0 ? o->nni_rounds : 0) : 0;
    const int64_t sprToDo = o && o->me_nni ? o->spr : 0;
    const int64_t mlNNIToDo = o && o->ml_nni ? veryfasttree::mlNNIRoundsToDo(nSeqs, o->ml_nni_rounds > 0 ? o->ml_nni_rounds : 0) : 0;
    for (double &x: gStage) x = 0;
    auto now = []() { return std::chrono::steady_clock::now(); };
    auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); };
    std::chrono::steady_clock::time_point t0 = now();
    if (o && o->intree) {   /* `-intree`: the topology is given, fastNJ does not run (VeryFastTreeImpl.tcc:124-141) */
        for (const std::string &w: tree.warnings) fprintf(stderr, "%s\n", w.c_str());
        drv.readTree(tree.parent.data(), tree.child.data(), tree.root, tree.nNodes);
        recordJoinCrc(drv.joins);   /* none */
    } else {
        recordJoinCrc(drv.run(-1));
        drv.finishRoot();
    }
    gStage[0] = since(t0);
    if (log) {
        drv.logTree("NJ");   /* VeryFastTreeImpl.tcc:143 */
        if (!(o && o->intree)) log->line("Initial topology in %.2f seconds", log->clock());   /* :150-153 */
        if (sprToDo > 0 || nniToDo > 0 || mlNNIToDo > 0)   /* :154-158 */
            log->line("Refining topology: %lld rounds ME-NNIs, %d rounds ME-SPRs, %lld rounds ML-NNIs", (long long) nniToDo, (int) sprToDo, (long long) mlNNIToDo);
    }
    static const bool stageTrace = std::getenv("VFT_STAGE_TRACE") != nullptr;   /* tools: the stages as they end, on stderr */
    if (stageTrace) fprintf(stderr, "[stage] NJ phase done after %.1f s\n", gStage[0]);
    t0 = now();
    if (o && o->me_nni) drv.meNNIRounds(o->spr);
    gStage[1] = since(t0);
    if (stageTrace) fprintf(stderr, "[stage] minimum-evolution NNIs + SPR done after %.1f s\n", gStage[1]);
    gStage[2] = drv.meSPRSeconds;
    t0 = now();
    if (meLengths) drv.updateBranchLengths();
    if (log && meLengths) {
        drv.logTree("ME_Lengths");   /* VeryFastTreeImpl.tcc:213 */
        log->line("Total branch-length %.3f after %.2f sec", drv.totalLen(), log->clock());   /* :215-220 */
    }
    const bool ml = o && (o->mllen || o->ml_nni);
    if (nBootstrap > 0 && !ml) drv.computeSupports(nBootstrap);
    gStage[3] = since(t0);
    t0 = now();
    if (ml) {
        if (!meLengths) throw std::invalid_argument("vft_nj_ml_newick: the ML stage needs me_lengths (updateBranchLengths runs first)");
        /* with supports: SH-like (testSplitsML) instead of the local bootstrap */
        const int32_t nCat = o->mllen ? o->mllen : (o->ml_nni > 1 ? o->ml_nni : 1);
        loglk = drv.mlLengths(nCat, nBootstrap, o->mllen != 0, o->ml_nni != 0, o->me_nni != 0, o->gtr != 0);
        if (gtrOut) {
            for (int i = 0; i < 6; i++) gtrOut[i] = drv.gtrRates[i];
            for (int i = 0; i < 4; i++) gtrOut[6 + i] = drv.gtrFreq[i];
        }
        rates.assign(drv.mlRates.begin(), drv.mlRates.end());
        ratecat = drv.mlRateCat;
    }
    gStage[4] = since(t0);
    gStage[5] = drv.mlNNISeconds;
    gStage[6] = drv.mlSupportSeconds;
    gStage[7] = drv.mlModelSeconds;
    for (int i = 0; i < 3; i++) gGamma[i] = drv.gammaFit[i];
    gLanes[0] = drv.mlLaneSteps;
    gLanes[1] = drv.mlLaneWork;
    gLanes[2] = drv.meSPRSteps;
    gLanes[3] = drv.meSPRs;
    gWalkDual[0] = drv.meSPRDualSent;
    gWalkDual[1] = drv.meSPRDualTaken;
    gLaneExchange[0] = drv.laneGathers;
    gLaneExchange[1] = drv.laneGatherBytes;
    drv.report();
    if (log) {   /* the summary (VeryFastTreeImpl.tcc:403-414, :425-450) */
        const int64_t bad = ml ? drv.mlBadSplits : drv.meBadSplits;
        const int64_t splits = ml ? drv.mlSplits : drv.meSplits;
        const double worst = ml ? drv.mlWorstDelta : drv.meWorstDelta;
        std::string total = veryfasttree::StageLog::format("Total time: %.2f seconds Unique: %lld/%lld Bad splits: %lld/%lld", log->clock(), (long long) nSeqs,
                                                           (long long) nAll, (long long) bad, (long long) splits);
        if (worst > 0) total += veryfasttree::StageLog::format(" Worst delta-%s %.3f", ml ? "LogLk" : "Len", worst);
        log->text(total + "\n");
        if (!(o && o->threads > 1) && (nniToDo > 0 || sprToDo > 0 || mlNNIToDo > 0))   /* :446-450: nothing of this block at more than one thread */
            log->line("NNI: %lld SPR: %lld ML-NNI: %lld", (long long) drv.meNNIs, (long long) drv.meSPRs, (long long) drv.mlNNIs);
    }
    const std::string text = drv.newick(nm, uf, an);
    if (log) log->line("TreeCompleted");   /* :469 */
    return text;
}

extern "C" int vft_nj_ml_newick(vft_ctx *ctx, const uint8_t *codes, int64_t nSeqs, int64_t nPos, int32_t precision,
                                const vft_nj_options *opt, int32_t meLengths, int32_t nBootstrap, const int64_t *uniqueFirst,
                                const int64_t *alnNext, int64_t nAll, const char *names, char *out, int64_t outCap,
                                int64_t *outLen, double *loglk, int32_t loglkCap, int32_t *nRounds, double *ratesOut,
                                int32_t ratesCap, int32_t *nRates, int32_t *ratecatOut, double *gtrOut, char *err, int32_t errLen) {
    if (!ctx || !codes || !uniqueFirst || !alnNext || !names || !outLen) return VFT_ERR_INVALID;
    try {
        /* The option checks come first and look at `opt` alone: ctx is not dereferenced before runTree.  Callers rely on a refusal
           reaching them with nothing uploaded, and the CPU tests (tests/test_thorough_cpu.py, tests/test_pseudo_cpu.py) hand over a
           context that is no context: a check that needs ctx goes below these, never between or above them. */
        checkIntree(opt, nSeqs);
        checkSlow(opt);
        checkPseudo(opt);
        checkThorough(opt);
        checkAAModel(opt);
        std::vector<double> ll, rates;
        std::vector<int64_t> ratecat;
        const std::string t = precision == 8 ? runTree<double>(ctx, codes, nSeqs, nPos, opt, meLengths != 0, nBootstrap, uniqueFirst, alnNext, nAll, names, ll, rates, ratecat, gtrOut)
                                             : runTree<float>(ctx, codes, nSeqs, nPos, opt, meLengths != 0, nBootstrap, uniqueFirst, alnNext, nAll, names, ll, rates, ratecat, gtrOut);
        if (nRates) *nRates = (int32_t) rates.size();
        if (ratesOut)
            for (size_t k = 0; k < rates.size() && (int32_t) k < ratesCap; k++) ratesOut[k] = rates[k];
        if (ratecatOut)
            for (size_t k = 0; k < ratecat.size(); k++) ratecatOut[k] = (int32_t) ratecat[k];
        if (nRounds) *nRounds = (int32_t) ll.size();
        if (loglk)
            for (size_t k = 0; k < ll.size() && (int32_t) k < loglkCap; k++) loglk[k] = ll[k];
        *outLen = (int64_t) t.size();
        if (out && outCap > (int64_t) t.size()) memcpy(out, t.c_str(), t.size() + 1);
        else if (out) return VFT_ERR_INVALID;   /* outLen tells how much is needed */
        return VFT_OK;
    } catch (const std::exception &e) {
        if (err && errLen > 0) snprintf(err, (size_t) errLen, "%s", e.what());
        return VFT_ERR_STATE;
    }
}

extern "C" int vft_nj_newick(vft_ctx *ctx, const uint8_t *codes, int64_t nSeqs, int64_t nPos, int32_t precision,
                             const vft_nj_options *opt, int32_t meLengths, int32_t nBootstrap, const int64_t *uniqueFirst, const int64_t *alnNext, int64_t nAll,
                             const char *names, char *out, int64_t outCap, int64_t *outLen, char *err, int32_t errLen) {
    vft_nj_options o;
    if (opt) {
        o = *opt;
        o.mllen = 0;
    }
    return vft_nj_ml_newick(ctx, codes, nSeqs, nPos, precision, opt ? &o : nullptr, meLengths, nBootstrap, uniqueFirst, alnNext,
                            nAll, names, out, outCap, outLen, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, err, errLen);
}

extern "C" void vft_knuth_stream(double *out, int64_t n) {
    veryfasttree::KnuthRng g;
    for (int64_t i = 0; i < n; i++) out[i] = g.rand();
}

template<typename REAL>
static int64_t runDriver(vft_ctx *ctx, const uint8_t *codes, int64_t nSeqs, int64_t nPos, const vft_nj_options *o,
                         int64_t maxJoins, int64_t *joins, double *criterion) {
    const veryfasttree::NJOptions opt = toOptions(o);
    veryfasttree::NJDriver<REAL> drv(ctx, codes, nSeqs, nPos, opt);
    const auto &js = drv.run(maxJoins);
    recordJoinCrc(js);
    drv.report();
    for (size_t k = 0; k < js.size(); k++) {
        joins[3 * k] = js[k].i;
        joins[3 * k + 1] = js[k].j;
        joins[3 * k + 2] = js[k].newnode;
        if (criterion) criterion[k] = js[k].criterion;
    }
    return (int64_t) js.size();
}

extern "C" int vft_nj_run(vft_ctx *ctx, const uint8_t *codes, int64_t nSeqs, int64_t nPos, int32_t precision,
                          const vft_nj_options *opt, int64_t maxJoins, int64_t *joins, double *criterion,
                          int64_t *nJoins, char *err, int32_t errLen) {
    if (!ctx || !codes || !joins || !nJoins) return VFT_ERR_INVALID;
    try {
        if (opt && opt->intree) throw std::invalid_argument("vft_nj_run returns the joins of the NJ phase: with -intree there are none (use vft_nj_newick)");
        checkSlow(opt);
        checkThorough(opt);
        *nJoins = precision == 8 ? runDriver<double>(ctx, codes, nSeqs, nPos, opt, maxJoins, joins, criterion)
                                 : runDriver<float>(ctx, codes, nSeqs, nPos, opt, maxJoins, joins, criterion);
        return VFT_OK;
    } catch (const std::exception &e) {
        if (err && errLen > 0) snprintf(err, (size_t) errLen, "%s", e.what());
        return VFT_ERR_STATE;
    }
}

template<typename REAL>
static void runMLLengths(vft_ctx *ctx, int64_t nSeqs, int64_t nNodes, int64_t nPos, const int64_t *parent, const int64_t *child,
                         int64_t root, void *bl, int32_t recomputeFirst, int32_t rounds, double ftol, double atol,
                         int64_t nLeafGaps, double *loglk, int64_t *evals) {
    veryfasttree::MLLengths<REAL> ml(ctx, nSeqs, nNodes, parent, child, root);
    ml.setLengths((const REAL *) bl);
    if (recomputeFirst & 1) ml.recomputeMLProfiles();
    for (int32_t r = 0; r < rounds; r++) {
        if (recomputeFirst & 2) ml.optimizeRoundParallel(ftol, atol);
        else ml.optimizeRound(ftol, atol);
        if (loglk) loglk[r] = ml.treeLogLk(nPos, nLeafGaps);
    }
    ml.getLengths((REAL *) bl);
    if (evals) *evals = ml.evaluations();
}

extern "C" int vft_ml_lengths(vft_ctx *ctx, int64_t nSeqs, int64_t nNodes, int64_t nPos, int32_t precision, const int64_t *parent,
                              const int64_t *child, int64_t root, void *bl, int32_t recomputeFirst, int32_t rounds, double ftol,
                              double atol, int64_t nLeafGaps, double *loglk, int64_t *evals, char *err, int32_t errLen) {
    if (!ctx || !parent || !child || !bl || nSeqs < 3 || nNodes <= nSeqs || rounds < 0) return VFT_ERR_INVALID;
    try {
        if (precision == 8) runMLLengths<double>(ctx, nSeqs, nNodes, nPos, parent, child, root, bl, recomputeFirst, rounds, ftol, atol, nLeafGaps, loglk, evals);
        else runMLLengths<float>(ctx, nSeqs, nNodes, nPos, parent, child, root, bl, recomputeFirst, rounds, ftol, atol, nLeafGaps, loglk, evals);
        return VFT_OK;
    } catch (const std::exception &e) {
        if (err && errLen > 0) snprintf(err, (size_t) errLen, "%s", e.what());
        return VFT_ERR_STATE;
    }
}

extern "C" int vft_gtr_tables(const double *rates, const double *freq, int32_t precision, double *stat, double *statinv, double *eigenval,
                              double *codefreq, double *eigeninv, double *eigeninvT) {
    if (!rates || !freq || !stat || !statinv || !eigenval || !codefreq || !eigeninv || !eigeninvT) return VFT_ERR_INVALID;
    try {
        veryfasttree::TransitionTables4 t;
        if (precision == 8) veryfasttree::createGTR<double>(rates, freq, t);
        else veryfasttree::createGTR<float>(rates, freq, t);
        for (int i = 0; i < 4; i++) {
            stat[i] = t.stat[i];
            statinv[i] = t.statinv[i];
            eigenval[i] = t.eigenval[i];
            for (int j = 0; j < 4; j++) {
                eigeninv[4 * i + j] = t.eigeninv[i][j];
                eigeninvT[4 * i + j] = t.eigeninvT[i][j];
            }
        }
        for (int i = 0; i < 5; i++)
            for (int j = 0; j < 4; j++) codefreq[4 * i + j] = t.codeFreq[i][j];
        return VFT_OK;
    } catch (const std::exception &) {
        return VFT_ERR_INVALID;
    }
}

template<typename REAL>
static void aaModelOut(const veryfasttree::TransitionTables20 &t, double *stat, double *statinv, double *eigenval, double *codefreq,
                       double *eigeninv, double *eigeninvT) {
    for (int i = 0; i < 20; i++) {
        stat[i] = t.stat[i];
        statinv[i] = t.statinv[i];
        eigenval[i] = t.eigenval[i];
        for (int j = 0; j < 20; j++) {
            eigeninv[20 * i + j] = t.eigeninv[i][j];
            eigeninvT[20 * i + j] = t.eigeninvT[i][j];
        }
    }
    for (int i = 0; i < 21; i++)
        for (int j = 0; j < 20; j++) codefreq[20 * i + j] = t.codeFreq[i][j];
}

extern "C" int vft_aa_model_tables(int32_t model, int32_t precision, double *stat, double *statinv, double *eigenval, double *codefreq,
                                   double *eigeninv, double *eigeninvT) {
    if (!stat || !statinv || !eigenval || !codefreq || !eigeninv || !eigeninvT) return VFT_ERR_INVALID;
    try {
        veryfasttree::TransitionTables20 t;
        if (precision == 8) veryfasttree::createAAModel<double>(model, t);
        else veryfasttree::createAAModel<float>(model, t);
        aaModelOut<double>(t, stat, statinv, eigenval, codefreq, eigeninv, eigeninvT);
        return VFT_OK;
    } catch (const std::exception &) {
        return VFT_ERR_INVALID;
    }
}

/* `-trans`: the parse alone (host/ReadTransition.h), no device and no file */
extern "C" int vft_read_aa_transition(const char *text, double *matrix, double *stat, char *err, int32_t errLen) {
    try {
        if (!text || !matrix || !stat) throw std::invalid_argument("vft_read_aa_transition: bad arguments");
        double m[20][20], s[20];
        veryfasttree::readAATransition(text, strlen(text), m, s);
        for (int i = 0; i < 20; i++) {
            stat[i] = s[i];
            for (int j = 0; j < 20; j++) matrix[20 * i + j] = m[i][j];
        }
        return VFT_OK;
    } catch (const std::exception &e) {
        if (err && errLen > 0) snprintf(err, (size_t) errLen, "%s", e.what());
        return VFT_ERR_INVALID;
    }
}

extern "C" int vft_nj_set_aa_transition(const double *matrix, const double *stat) {
    veryfasttree::AATransition &custom = veryfasttree::customAATransition();
    if (!matrix && !stat) {
        custom.set = false;
        return VFT_OK;
    }
    if (!matrix || !stat) return VFT_ERR_INVALID;
    for (int i = 0; i < 20; i++)
        if (!(stat[i] > 0) || !std::isfinite(stat[i])) return VFT_ERR_INVALID;   /* (1 / stat and sqrt(stat) are taken) */
    for (int i = 0; i < 400; i++)
        if (!std::isfinite(matrix[i])) return VFT_ERR_INVALID;
    for (int i = 0; i < 20; i++) {
        custom.stat[i] = stat[i];
        for (int j = 0; j < 20; j++) custom.matrix[i][j] = matrix[20 * i + j];
    }
    custom.set = true;
    return VFT_OK;
}

extern "C" int vft_nj_get_aa_transition(void) { return veryfasttree::customAATransition().set ? 1 : 0; }

extern "C" int vft_aa_model_matrix(int32_t model, double *matrix, double *stat) {
    if (!matrix || !stat) return VFT_ERR_INVALID;
    try {
        const double *s, *flat;
        veryfasttree::aaModelConstants(model, s, flat);
        for (int i = 0; i < 20; i++) stat[i] = s[i];
        for (int i = 0; i < 400; i++) matrix[i] = flat[i];
        return VFT_OK;
    } catch (const std::exception &) {
        return VFT_ERR_INVALID;
    }
}

template<typename REAL>
static void tablesFromMatrix(const double *matrix, const double *stat, veryfasttree::TransitionTables20 &t) {
    double m[20][20];
    for (int i = 0; i < 20; i++)
        for (int j = 0; j < 20; j++) m[i][j] = matrix[20 * i + j];
    veryfasttree::createTransitionTables<REAL, 20>(m, stat, t);
}

extern "C" int vft_aa_tables_from_matrix(const double *matrix, const double *statIn, int32_t precision, double *stat, double *statinv, double *eigenval,
                                         double *codefreq, double *eigeninv, double *eigeninvT) {
    if (!matrix || !statIn || !stat || !statinv || !eigenval || !codefreq || !eigeninv || !eigeninvT || (precision != 4 && precision != 8)) return VFT_ERR_INVALID;
    try {
        veryfasttree::TransitionTables20 t;
        if (precision == 8) tablesFromMatrix<double>(matrix, statIn, t);
        else tablesFromMatrix<float>(matrix, statIn, t);
        aaModelOut<double>(t, stat, statinv, eigenval, codefreq, eigeninv, eigeninvT);
        return VFT_OK;
    } catch (const std::exception &) {
        return VFT_ERR_INVALID;
    }
}

extern "C" int vft_aa_near_tables_from_matrix(const double *matrix, const double *statIn, int32_t precision, double *nearP, double *nearFreq) {
    if (!matrix || !statIn || !nearP || !nearFreq || (precision != 4 && precision != 8)) return VFT_ERR_INVALID;
    try {
        veryfasttree::TransitionTables20 t;
        veryfasttree::NearTables20 n;
        if (precision == 8) {
            tablesFromMatrix<double>(matrix, statIn, t);
            veryfasttree::nearPosteriorTables<double>(t, n);
        } else {
            tablesFromMatrix<float>(matrix, statIn, t);
            veryfasttree::nearPosteriorTables<float>(t, n);
        }
        for (int i = 0; i < 20; i++)
            for (int j = 0; j < 20; j++) {
                nearP[20 * i + j] = n.nearP[i][j];
                nearFreq[20 * i + j] = n.nearFreq[i][j];
            }
        return VFT_OK;
    } catch (const std::exception &) {
        return VFT_ERR_INVALID;
    }
}

extern "C" int vft_aa_near_tables(int32_t model, int32_t precision, double *nearP, double *nearFreq) {
    if (!nearP || !nearFreq || (precision != 4 && precision != 8)) return VFT_ERR_INVALID;
    try {
        veryfasttree::TransitionTables20 t;
        veryfasttree::NearTables20 n;
        if (precision == 8) {
            veryfasttree::createAAModel<double>(model, t);
            veryfasttree::nearPosteriorTables<double>(t, n);
        } else {
            veryfasttree::createAAModel<float>(model, t);
            veryfasttree::nearPosteriorTables<float>(t, n);
        }
        for (int i = 0; i < 20; i++)
            for (int j = 0; j < 20; j++) {
                nearP[20 * i + j] = n.nearP[i][j];
                nearFreq[20 * i + j] = n.nearFreq[i][j];
            }
        return VFT_OK;
    } catch (const std::exception &) {
        return VFT_ERR_INVALID;
    }
}

static void distanceTablesOut(const veryfasttree::DistanceTables20 &d, double *distances, double *codefreq, double *eigenval,
                              double *eigentot) {
    for (int i = 0; i < 20; i++) {
        eigenval[i] = d.eigenval[i];
        eigentot[i] = d.eigentot[i];
        for (int j = 0; j < 20; j++) {
            distances[20 * i + j] = d.distances[i][j];
            codefreq[20 * i + j] = d.codeFreq[i][j];
        }
    }
}

extern "C" int vft_blosum45_tables(int32_t precision, double *distances, double *codefreq, double *eigenval, double *eigentot) {
    if (!distances || !codefreq || !eigenval || !eigentot) return VFT_ERR_INVALID;
    veryfasttree::DistanceTables20 d;
    if (precision == 8) veryfasttree::blosum45Tables<double>(d);
    else veryfasttree::blosum45Tables<float>(d);
    distanceTablesOut(d, distances, codefreq, eigenval, eigentot);
    return VFT_OK;
}

extern "C" int vft_aa_model_as_distance_tables(int32_t model, int32_t precision, double *distances, double *codefreq,
                                               double *eigenval, double *eigentot) {
    if (!distances || !codefreq || !eigenval || !eigentot) return VFT_ERR_INVALID;
    try {
        veryfasttree::TransitionTables20 t;
        veryfasttree::DistanceTables20 d;
        if (precision == 8) {
            veryfasttree::createAAModel<double>(model, t);
            veryfasttree::transitionAsDistanceTables<double>(t, d);
        } else {
            veryfasttree::createAAModel<float>(model, t);
            veryfasttree::transitionAsDistanceTables<float>(t, d);
        }
        distanceTablesOut(d, distances, codefreq, eigenval, eigentot);
        return VFT_OK;
    } catch (const std::exception &) {
        return VFT_ERR_INVALID;
    }
}

template <typename REAL>
static veryfasttree::SeqMatrixTimes runMakeMatrix(vft_ctx *ctx, int64_t nSeqs, const std::vector<std::string> &names, bool logCorrect,
                                                  int64_t slabRows, int fd) {
    veryfasttree::DeviceSlabs<REAL> slabs(ctx, nSeqs, slabRows, logCorrect);
    return veryfasttree::writeSeqMatrix<REAL>(slabs, nSeqs, names, slabs.slabRows(), fd);
}

extern "C" int vft_nj_make_matrix(vft_ctx *ctx, int64_t nSeqs, int32_t precision, const char *names, int32_t logCorrect, int64_t slabRows,
                                  int32_t fd, const vft_comm *comm, double *seconds, int64_t *counts, char *err, int32_t errLen) {
    try {
        if (!ctx || !names || nSeqs < 1 || fd < 0 || (precision != 4 && precision != 8)) throw std::runtime_error("vft_nj_make_matrix: bad arguments");
        if (comm && comm->world > 1)
            throw std::runtime_error("-makematrix runs on one GPU: the matrix is not split over the ranks of a communicator (and is not approximated)");
        openLog(comm);   /* `-makematrix` writes the log's first line and nothing else */
        std::vector<std::string> nm;
        const char *p = names;
        for (int64_t k = 0; k < nSeqs; k++) {
            nm.emplace_back(p);
            p += nm.back().size() + 1;
        }
        const veryfasttree::SeqMatrixTimes T = precision == 4 ? runMakeMatrix<float>(ctx, nSeqs, nm, logCorrect != 0, slabRows, fd)
                                                              : runMakeMatrix<double>(ctx, nSeqs, nm, logCorrect != 0, slabRows, fd);
        if (seconds) {
            seconds[0] = T.wait;
            seconds[1] = T.format;
            seconds[2] = T.write;
            seconds[3] = T.total;
        }
        if (counts) {
            counts[0] = T.slabs;
            counts[1] = T.slabRows;
            counts[2] = T.bytes;
        }
        return VFT_OK;
    } catch (const std::exception &e) {
        if (err && errLen > 0) snprintf(err, (size_t) errLen, "%s", e.what());
        return VFT_ERR_INVALID;
    }
}
