// `-log FILE`: the sink of the reference's log lines.  Plain C++11, no HIP.
//
// One StageLog per run, handed to NJDriver and MLLengths by pointer; a null pointer is "no log": the caller formats nothing and
// tracks nothing.  Every line goes out with write(2) as soon as its stage has finished, so a run that fails leaves the lines of
// the stages it completed.  A write error is an error of the run (std::runtime_error naming the log).
#ifndef VFT_STAGE_LOG_H
#define VFT_STAGE_LOG_H

#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unistd.h>

namespace veryfasttree {

    class StageLog {
    public:
        explicit StageLog(int fd) : fd(fd), t0(std::chrono::steady_clock::now()) {}

        /* progressReport.clockDiff(): seconds since the run began */
        double clock() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

        /* the text as it stands (the caller ends its lines) */
        void text(const std::string &s) {
            const char *p = s.data();
            size_t left = s.size();
            while (left > 0) {
                const ssize_t n = ::write(fd, p, left);
                if (n < 0) {
                    if (errno == EINTR) continue;
                    throw std::runtime_error(std::string("-log: writing the log failed: ") + strerror(errno));
                }
                p += n;
                left -= (size_t) n;
            }
        }

        /* one formatted line; the newline is added here */
        void line(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
            va_list ap;
            va_start(ap, fmt);
            std::string s = vformat(fmt, ap);
            va_end(ap);
            text(s + "\n");
        }

        static std::string format(const char *fmt, ...) __attribute__((format(printf, 1, 2))) {
            va_list ap;
            va_start(ap, fmt);
            const std::string s = vformat(fmt, ap);
            va_end(ap);
            return s;
        }

        static std::string vformat(const char *fmt, va_list ap) {
            va_list ap2;
            va_copy(ap2, ap);
            const int n = vsnprintf(nullptr, 0, fmt, ap2);
            va_end(ap2);
            std::string s((size_t) (n > 0 ? n : 0), '\0');
            if (n > 0) vsnprintf(&s[0], (size_t) n + 1, fmt, ap);
            return s;
        }

    private:
        int fd;
        std::chrono::steady_clock::time_point t0;
    };

}

#endif
