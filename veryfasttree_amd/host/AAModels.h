// Amino-acid models as the reference sets them up, on the host: the three built-in exchange matrices
// (createTransitionMatrixJTT92 / WAG01 / LG08, TransitionMatrix.tcc:14-24 -> createTransitionMatrix :158-232), the
// default BLOSUM45-derived distance matrix of the NJ / minimum-evolution phase (matrixBLOSUM45 + setupDistanceMatrix,
// DistanceMatrix.tcc:33-36, 102-155) and the transition matrix re-expressed as a "distance matrix" for re-averaging
// the profiles before the ML phase (transMatToDistanceMat, VeryFastTreeImpl.tcc:517-542).  The constants live in
// AAModelData.h (generated); the tables cross the boundary through vft_set_transition_matrix / vft_set_distance_matrix.
#ifndef VFT_AA_MODELS_H
#define VFT_AA_MODELS_H

#include <stdexcept>

#include "AAModelData.h"
#include "GtrModel.h"

namespace veryfasttree {

    enum AAModel {
        AA_MODEL_JTT = 1,   /* the reference's default for amino acids (VeryFastTreeImpl.tcc:104-106) */
        AA_MODEL_WAG = 2,   /* -wag */
        AA_MODEL_LG = 3,    /* -lg */
        AA_MODEL_CUSTOM = 4 /* -trans FILE: the matrix that was set (customAATransition below) */
    };

    /* `-trans`: the user's rate matrix and stationary frequencies (host/ReadTransition.h), process state like the log's descriptor:
       set by vft_nj_set_aa_transition, read by createAAModel(AA_MODEL_CUSTOM), cleared by the same call with NULL - never by a run */
    struct AATransition {
        bool set;
        double matrix[20][20], stat[20];
    };
    inline AATransition &customAATransition() {
        static AATransition custom = {false, {{0}}, {0}};
        return custom;
    }

    /* a built-in model's constants as they stand in AAModelData.h (vft_aa_model_matrix) */
    inline void aaModelConstants(int model, const double *&stat, const double *&flat) {
        switch (model) {
            case AA_MODEL_JTT:
                stat = aa_data::kStatJTT92;
                flat = aa_data::kMatrixJTT92;
                break;
            case AA_MODEL_WAG:
                stat = aa_data::kStatWAG01;
                flat = aa_data::kMatrixWAG01;
                break;
            case AA_MODEL_LG:
                stat = aa_data::kStatLG08;
                flat = aa_data::kMatrixLG08;
                break;
            default:
                throw std::invalid_argument("unknown amino-acid model (1 = JTT, 2 = WAG, 3 = LG)");
        }
    }

    typedef TransitionTables<20> TransitionTables20;

    /* what vft_set_distance_matrix takes: numeric_t values held in double */
    struct DistanceTables20 {
        double distances[20][20], codeFreq[20][20], eigenval[20], eigentot[20];
    };

    template<typename REAL>
    inline void createAAModel(int model, TransitionTables20 &t) {
        if (model == AA_MODEL_CUSTOM) {
            const AATransition &custom = customAATransition();
            if (!custom.set) throw std::invalid_argument("amino-acid model 4 (-trans) without a matrix: vft_nj_set_aa_transition comes first");
            createTransitionTables<REAL, 20>(custom.matrix, custom.stat, t);
            return;
        }
        const double *stat, *flat;
        aaModelConstants(model, stat, flat);
        double matrix[20][20];
        for (int i = 0; i < 20; i++)
            for (int j = 0; j < 20; j++) matrix[i][j] = flat[20 * i + j];
        createTransitionTables<REAL, 20>(matrix, stat, t);
    }

    /* what vft_set_near_posteriors takes: numeric_t values held in double */
    struct NearTables20 {
        double nearP[20][20], nearFreq[20][20];
    };

    /* The tail of createTransitionMatrix (TransitionMatrix.tcc:227-279), `-approxml`'s near-constant posteriors: P(t = approxMLnearT)
       from the STORED (numeric_t) tables in double, nearP[i][j] ~ stat[j] * P(j -> i | t)^2 normalised, nearFreq[i] = nearP[i] / stat
       rotated by codeFreq - statement for statement in the reference's order, with the host's exp (the rotation's inner product
       reads codeFreq[i][j] for every k, as the reference's does) */
    template<typename REAL>
    inline void nearPosteriorTables(const TransitionTables20 &t, NearTables20 &n) {
        const double nearT = 0.2;   /* Constants::approxMLnearT */
        double expvalues[20], LVinv[20][20], transt[20][20];
        for (int i = 0; i < 20; i++) expvalues[i] = std::exp(nearT * t.eigenval[i]);
        for (int i = 0; i < 20; i++)
            for (int j = 0; j < 20; j++) LVinv[i][j] = t.eigeninv[i][j] * expvalues[i];
        for (int i = 0; i < 20; i++)
            for (int j = 0; j < 20; j++) {
                transt[i][j] = 0;
                for (int k = 0; k < 20; k++) transt[i][j] += t.codeFreq[i][k] * LVinv[k][j];
            }
        for (int i = 0; i < 20; i++) {
            double p[20], tot = 0;
            for (int j = 0; j < 20; j++) {
                p[j] = t.stat[j] * transt[i][j] * transt[i][j];
                tot += p[j];
            }
            for (int j = 0; j < 20; j++) p[j] *= 1.0 / tot;
            for (int j = 0; j < 20; j++) n.nearP[i][j] = (double) (REAL) p[j];
            for (int j = 0; j < 20; j++) p[j] /= t.stat[j];
            for (int j = 0; j < 20; j++) {
                double rot = 0;
                for (int k = 0; k < 20; k++) rot += p[k] * t.codeFreq[i][j];
                n.nearFreq[i][j] = (double) (REAL) rot;
            }
        }
    }

    /* matrixBLOSUM45 + setupDistanceMatrix: the literals are narrowed to numeric_t where the reference's static
       initialiser narrows them; eigentot is summed in numeric_t (DistanceMatrix.tcc:127-133), codeFreq is the
       transpose of eigeninv (:135-140) */
    template<typename REAL>
    inline void blosum45Tables(DistanceTables20 &d) {
        REAL eigeninv[20][20];
        for (int i = 0; i < 20; i++) {
            d.eigenval[i] = (double) (REAL) aa_data::kBlosum45EigenVal[i];
            for (int j = 0; j < 20; j++) {
                d.distances[i][j] = (double) (REAL) aa_data::kBlosum45Distances[20 * i + j];
                eigeninv[i][j] = (REAL) aa_data::kBlosum45EigenInv[20 * i + j];
            }
        }
        for (int k = 0; k < 20; k++) {
            REAL tot = 0;
            for (int j = 0; j < 20; j++) tot += eigeninv[k][j];
            d.eigentot[k] = (double) tot;
        }
        for (int code = 0; code < 20; code++)
            for (int k = 0; k < 20; k++) d.codeFreq[code][k] = (double) eigeninv[k][code];
    }

    /* transMatToDistanceMat: rotation and normalisation of the transition matrix in the DistanceMatrix slots; the
       distances ("never actually used") and the eigenvalues stay zero as in the reference's value-initialised object */
    template<typename REAL>
    inline void transitionAsDistanceTables(const TransitionTables20 &t, DistanceTables20 &d) {
        for (int i = 0; i < 20; i++) {
            d.eigenval[i] = 0;
            REAL tot = 0;
            for (int j = 0; j < 20; j++) {
                d.distances[i][j] = 0;
                d.codeFreq[i][j] = t.codeFreq[i][j];
                tot += (REAL) t.eigeninv[i][j];
            }
            d.eigentot[i] = (double) tot;
        }
    }

}

#endif
