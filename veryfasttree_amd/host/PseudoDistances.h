/* correctedPairDistances behind profileDist (NJ.tcc:1460-1488): the pseudocount estimate of `-pseudo` and the log correction
   (logCorrect, NJ.tcc:322-330) for the 3 pairs of a triplet (AB AC BC) or the 6 of a quartet (AB AC AD BC BD CD).  The one place
   that arithmetic lives: updateBranchLengths (NJDriver.h), the lockstep lanes and the one-thread walks (MLLengths.h) all come here
   with the numeric_t distances and weights vft_profile_distances / the walk server returned; exported as vft_pseudo_distances.

     dTop    = sum dist_k * weight_k     the product of two numeric_t IN numeric_t (a float product in a float run), widened, added in pair order
     dBottom = sum weight_k              double, in pair order
     prior   = dBottom > 0.01 ? dTop / dBottom : 3.0
     d_k     = ((double) dist_k * weight_k + prior * pseudoWeight) / (weight_k + pseudoWeight)      all double

   `correction` (DistCorrection below) is what happens to d_k last: Jukes-Cantor, scoredist-like, or - `-rawdist` - nothing.
   pseudoWeight == 0: the log-corrected distances alone, the weights are not read (weight may be NULL).  Built without FMA
   contraction like the rest of the host library (the reference is -O3 -mavx2 without -mfma): the numeric_t product stays one. */
#ifndef VFT_HOST_PSEUDO_DISTANCES_H
#define VFT_HOST_PSEUDO_DISTANCES_H

#include <cmath>

namespace veryfasttree {

    /* What a distance goes through behind the pseudocounts: logCorrect's two formulas (NJ.tcc:322-330), or nothing - `-rawdist`, the
       `if (options.logdist)` around the correction (NJ.tcc:1484).  The first two are 0 and 1, the values of the `scoredist` arguments
       of the C ABI (vft_pseudo_distances, vft_walk_scoredist), which keep their meaning; the third has no value there. */
    enum DistCorrection {
        DIST_JUKES_CANTOR = 0,
        DIST_SCOREDIST = 1,
        DIST_RAW = 2
    };

    /* The one place that decides it for a run of the driver: `rawDistances` is the context's switch (vft_get_raw_distances), `scoredist`
       the options' (amino acids / a distance matrix).  NJDriver and, through it, MLLengths read this and nothing else. */
    inline int distCorrectionOf(bool rawDistances, bool scoredist) {
        return rawDistances ? DIST_RAW : scoredist ? DIST_SCOREDIST : DIST_JUKES_CANTOR;
    }

    inline double pseudoLogCorrect(double dist, int correction) {   /* NJ.tcc:322-330 */
        const double maxscore = 3.0;
        if (correction == DIST_RAW) return dist;
        if (correction == DIST_JUKES_CANTOR) dist = dist < 0.74 ? -0.75 * std::log(1.0 - dist * 4.0 / 3.0) : maxscore;   /* Jukes-Cantor */
        else dist = dist < 0.99 ? -1.3 * std::log(1.0 - dist) : maxscore;                          /* scoredist-like */
        return dist < maxscore ? dist : maxscore;
    }

    /* ... for weights as the DEVICE answers them (vft_profile_distances, the walk server): for two leaves that is seqDist's weight
       (NJ.tcc:1618), the number of common columns - 0 for a pair without one, where correctedPairDistances, which calls profileDist on
       leaves too, sees Besthit::weight = 0.01 (NJ.tcc:1187).  Everywhere else the two agree (a common column of two leaves weighs 1). */
    template<typename REAL>
    inline void pseudoDistances(int nPairs, const REAL *dist, const REAL *weight, double pseudoWeight, int correction, double *out);
    template<typename REAL>
    inline void pseudoDistancesOfDevice(int nPairs, const REAL *dist, const REAL *weight, double pseudoWeight, int correction, double *out) {
        REAL w[6] = {0, 0, 0, 0, 0, 0};
        if (pseudoWeight > 0)
            for (int k = 0; k < nPairs && k < 6; k++) w[k] = weight[k] > 0 ? weight[k] : (REAL) 0.01;
        pseudoDistances<REAL>(nPairs, dist, w, pseudoWeight, correction, out);
    }

    template<typename REAL>
    inline void pseudoDistances(int nPairs, const REAL *dist, const REAL *weight, double pseudoWeight, int correction, double *out) {
        for (int k = 0; k < nPairs; k++) out[k] = (double) dist[k];
        if (pseudoWeight > 0) {
            double dTop = 0, dBottom = 0;
            for (int k = 0; k < nPairs; k++) {
                const volatile REAL prod = dist[k] * weight[k];   /* rounded to numeric_t before it is widened */
                dTop += (double) prod;
                dBottom += (double) weight[k];
            }
            const double prior = dBottom > 0.01 ? dTop / dBottom : 3.0;
            for (int k = 0; k < nPairs; k++) out[k] = (out[k] * (double) weight[k] + prior * pseudoWeight) / ((double) weight[k] + pseudoWeight);
        }
        for (int k = 0; k < nPairs; k++) out[k] = pseudoLogCorrect(out[k], correction);
    }

}

#endif
