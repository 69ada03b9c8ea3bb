/* `-trans FILE`: a user's amino-acid rate matrix as the reference reads it (readAATransitionMatrix, TransitionMatrix.tcc:63-156).
   Pure host code, no device, no file: the caller hands over the file's text (exported as vft_read_aa_transition).

     line 1        A<tab>R<tab>N ... <tab>V<tab>*          the twenty codes in the alphabet's order, then a star
     lines 2-21    the code, its 20 rates (row i, column j), its stationary frequency - tab-separated; what follows the 22nd
                   field of a line, and every line behind the 21st, is not read

   Lines end at '\n', a '\r' in front of it is dropped (Utils.h readline).  A number is what std::stod makes of the field: leading
   blanks and a tail that is no number are accepted, as there.  Where the reference lets std::stod throw on a field that holds no
   number at all, the message here names the amino acid.  The checks, at tolerance 1e-5, and their texts are the reference's:
   every frequency at least the tolerance, their sum 1; every diagonal below minus the tolerance, the diagonal's dot product with the
   frequencies -1; no negative off-diagonal entry; every column's sum 0.  matrix[i][j] is the rate of row i, column j as written:
   createTransitionTables (GtrModel.h) sets the diagonal from the column sums itself. */
#ifndef VFT_HOST_READ_TRANSITION_H
#define VFT_HOST_READ_TRANSITION_H

#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>

namespace veryfasttree {

    namespace read_transition_detail {
        static const char kCodesAA[] = "ARNDCQEGHILKMFPSTWYV";

        inline std::string msg(const char *fmt, char a, char b = 0) {
            char buf[256];
            snprintf(buf, sizeof(buf), fmt, a, b);   /* (formats of one %c leave b alone) */
            return std::string(buf);
        }

        inline std::string number(const char *fmt, double x) {
            char buf[256];
            snprintf(buf, sizeof(buf), fmt, x);
            return std::string(buf);
        }

        /* the next line of text[pos, len), without its end; false behind the last one (a text that ends in '\n' has an empty last
           line, as std::getline followed by an eof() test sees it) */
        inline bool nextLine(const char *text, size_t len, size_t &pos, bool &atEnd, std::string &line) {
            if (atEnd) return false;
            size_t e = pos;
            while (e < len && text[e] != '\n') e++;
            line.assign(text + pos, e - pos);
            if (e >= len) atEnd = true;   /* getline met the end of the stream: eofbit */
            pos = e < len ? e + 1 : len;
            if (!line.empty() && line[line.size() - 1] == '\r') line.resize(line.size() - 1);
            return true;
        }

        /* the next tab-separated field of line[pos, ...); false when the line is used up (std::getline on a string stream: an empty
           field in front of a tab is a field, nothing behind the last character is none) */
        inline bool nextField(const std::string &line, size_t &pos, std::string &field) {
            if (pos >= line.size()) return false;
            size_t e = line.find('\t', pos);
            if (e == std::string::npos) e = line.size();
            field.assign(line, pos, e - pos);
            pos = e + 1;
            return true;
        }

        inline double numberOf(const std::string &field, char aa) {
            try {
                return std::stod(field);
            } catch (const std::exception &) {
                throw std::invalid_argument(std::string("Field '") + field + "' for amino acid " + aa + " is not a number");
            }
        }
    }

    inline void readAATransition(const char *text, size_t len, double matrix[20][20], double stat[20]) {
        using namespace read_transition_detail;
        std::string expected;
        for (int i = 0; i < 20; i++) {
            expected += kCodesAA[i];
            expected += '\t';
        }
        expected += '*';
        size_t pos = 0;
        bool atEnd = false;
        std::string line, field;
        if (!nextLine(text, len, pos, atEnd, line)) throw std::invalid_argument("Error reading header line from transition matrix file");
        if (line != expected) throw std::invalid_argument("Invalid header line in transition matrix file, it must match: " + expected);
        for (int i = 0; i < 20; i++) {
            const char aa = kCodesAA[i];
            if (!nextLine(text, len, pos, atEnd, line)) throw std::invalid_argument("Error reading matrix line");
            size_t at = 0;
            if (!nextField(line, at, field) || field.size() != 1 || field[0] != aa)
                throw std::invalid_argument(msg("Line for amino acid %c does not have the expected beginning", aa));
            for (int j = 0; j <= 20; j++) {   /* 20 rates, then the stationary frequency */
                if (!nextField(line, at, field)) throw std::invalid_argument(msg("Not enough fields for amino acid %c", aa));
                (j < 20 ? matrix[i][j] : stat[i]) = numberOf(field, aa);
            }
        }
        const double tol = 1e-5;
        double statTot = 0;
        for (int i = 0; i < 20; i++) {
            if (stat[i] < tol) throw std::invalid_argument(msg("stationary frequency for amino acid %c must be positive", kCodesAA[i]));
            statTot += stat[i];
        }
        if (std::fabs(statTot - 1) > tol) throw std::invalid_argument(number("stationary frequencies must sum to 1 -- actual sum is %g", statTot));
        double totRate = 0;
        for (int i = 0; i < 20; i++) {
            const double diag = matrix[i][i];
            if (diag > -tol) throw std::invalid_argument(msg("transition rate(%c,%c) must be negative", kCodesAA[i], kCodesAA[i]));
            totRate += stat[i] * diag;
        }
        if (std::fabs(totRate + 1) > tol)
            throw std::invalid_argument(number("Dot product of matrix diagonal and stationary frequencies must be -1 -- actual dot product is %g", totRate));
        for (int j = 0; j < 20; j++) {
            double colSum = 0;
            for (int i = 0; i < 20; i++) {
                const double value = matrix[i][j];
                colSum += value;
                if (i != j && value < 0) throw std::invalid_argument(msg("Off-diagonal matrix entry for (%c,%c) is negative", kCodesAA[i], kCodesAA[j]));
            }
            if (std::fabs(colSum) > tol) {
                char buf[256];
                snprintf(buf, sizeof(buf), "Sum of column %c must be zero -- actual sum is %g", kCodesAA[j], colSum);
                throw std::invalid_argument(buf);
            }
        }
    }

}

#endif
