// bindfx.h — the file effects of a bind (PreStart) and of a GC pass, as plain
// POSIX calls: the two per-allocation symlinks, the limits file written to a
// temp name and renamed, and the unlinks of a GC pass. Header-only and free
// of pybind, like wirecore.h and h2frame.h, so the stand-alone self-test
// (bindfx_selftest.cpp) covers exactly what _fastwire exports; the module
// calls these with the GIL released.
//
// Failures throw SysError carrying the errno and the path it belongs to; the
// module turns that into OSError (so ENOENT is FileNotFoundError in Python).
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace bindfx {

struct SysError : std::runtime_error {
  int err;
  std::string path;
  SysError(int e, const std::string& p)
      : std::runtime_error(p + ": " + strerror(e)), err(e), path(p) {}
};

constexpr int kLinkTries = 5;

// One (target, link) pair, GPUOperator._force_symlink's contract: a link that
// already has the target counts as made; anything else at the path is
// unlinked and the symlink tried again, kLinkTries times at the most
// (concurrent binds of one device-set hash and GC passes create and unlink
// the same link). Then EEXIST.
inline void force_symlink(const std::string& target, const std::string& link) {
  std::string have;
  for (int i = 0; i < kLinkTries; ++i) {
    if (symlink(target.c_str(), link.c_str()) == 0) return;
    if (errno != EEXIST) throw SysError(errno, link);
    // one byte more than the target: a longer link must not compare equal
    have.resize(target.size() + 1);
    ssize_t n = readlink(link.c_str(), &have[0], have.size());
    if (n == (ssize_t)target.size() && memcmp(have.data(), target.data(), target.size()) == 0)
      return;
    if (unlink(link.c_str()) != 0 && errno != ENOENT) throw SysError(errno, link);
  }
  throw SysError(EEXIST, link);
}

inline void make_links(const std::vector<std::pair<std::string, std::string>>& pairs) {
  for (auto& p : pairs) force_symlink(p.first, p.second);
}

// `data` to `path` through a temp file in the same directory and a rename,
// so a reader sees the old bytes or the new ones, never a part. The temp
// name is <path>.<pid>.<counter>.tmp: unique among this process's threads by
// the counter and among processes by the pid, and O_EXCL refuses a leftover
// of a dead process with a recycled pid (the counter then moves on). No
// fsync, as the Python writer before it. On any failure the temp file is
// unlinked.
inline void atomic_write(const std::string& path, const char* data, size_t len) {
  static std::atomic<unsigned long long> counter{0};
  std::string tmp;
  int fd = -1;
  for (int i = 0; i < 100; ++i) {
    char suffix[64];
    snprintf(suffix, sizeof suffix, ".%ld.%llu.tmp", (long)getpid(),
             counter.fetch_add(1, std::memory_order_relaxed));
    tmp = path + suffix;
    fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0600);
    if (fd >= 0 || errno != EEXIST) break;
  }
  if (fd < 0) throw SysError(errno, tmp);
  size_t off = 0;
  while (off < len) {
    ssize_t n = write(fd, data + off, len - off);
    if (n < 0) {
      if (errno == EINTR) continue;
      const int e = errno;
      close(fd);
      unlink(tmp.c_str());
      throw SysError(e, tmp);
    }
    off += (size_t)n;
  }
  // the descriptor is gone after close() whatever it returns: no retry
  if (close(fd) != 0 && errno != EINTR) {
    const int e = errno;
    unlink(tmp.c_str());
    throw SysError(e, tmp);
  }
  if (rename(tmp.c_str(), path.c_str()) != 0) {
    const int e = errno;
    unlink(tmp.c_str());
    throw SysError(e, path);
  }
}

// unlink every path; ENOENT is not an error. All are tried; the first other
// failure is thrown afterwards.
inline void unlink_many(const std::vector<std::string>& paths) {
  int first_err = 0;
  const std::string* first_path = nullptr;
  for (auto& p : paths) {
    if (unlink(p.c_str()) != 0 && errno != ENOENT && !first_err) {
      first_err = errno;
      first_path = &p;
    }
  }
  if (first_err) throw SysError(first_err, *first_path);
}

}  // namespace bindfx
