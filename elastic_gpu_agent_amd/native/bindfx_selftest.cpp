// Stand-alone check of bindfx.h (make_links, atomic_write, unlink_many), meant
// to be built with -fsanitize=address,undefined and run directly (the pybind
// modules themselves are never run under a sanitizer). Works in a directory
// of its own under $TMPDIR (or /tmp) and removes it.
//
// Build + run: python -m elastic_gpu_agent_amd.native.build_fuzz --selftest
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "bindfx.h"

namespace {

std::atomic<int> failures{0};

#define CHECK(cond, what)                                                          \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, what);    \
      ++failures;                                                                  \
    }                                                                              \
  } while (0)

std::string root;

std::vector<std::string> listing(const std::string& dir) {
  std::vector<std::string> out;
  DIR* d = opendir(dir.c_str());
  if (!d) return out;
  while (dirent* e = readdir(d)) {
    std::string n = e->d_name;
    if (n != "." && n != "..") out.push_back(n);
  }
  closedir(d);
  return out;
}

std::string link_target(const std::string& p) {
  char buf[512];
  ssize_t n = readlink(p.c_str(), buf, sizeof buf);
  return n < 0 ? std::string("<none>") : std::string(buf, (size_t)n);
}

std::string slurp(const std::string& p) {
  std::string out;
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) return "<unreadable>";
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
  fclose(f);
  return out;
}

void spit(const std::string& p, const std::string& data) {
  FILE* f = fopen(p.c_str(), "wb");
  fwrite(data.data(), 1, data.size(), f);
  fclose(f);
}

int err_of(void (*fn)(const std::string&), const std::string& arg) {
  try {
    fn(arg);
  } catch (const bindfx::SysError& e) {
    return e.err;
  }
  return 0;
}

void test_links() {
  const std::string gpu = root + "/elastic-gpu-x-0", ctl = root + "/elastic-gpuctl-x-0";
  const std::vector<std::pair<std::string, std::string>> pairs = {
      {"/dev/dri/renderD128", gpu}, {"/dev/kfd", ctl}};
  bindfx::make_links(pairs);  // fresh
  CHECK(link_target(gpu) == "/dev/dri/renderD128" && link_target(ctl) == "/dev/kfd", "fresh");
  struct stat a, b;
  lstat(gpu.c_str(), &a);
  bindfx::make_links(pairs);  // already correct: left alone
  lstat(gpu.c_str(), &b);
  CHECK(a.st_ino == b.st_ino, "kept");
  unlink(gpu.c_str());
  CHECK(symlink("/dev/dri/renderD129", gpu.c_str()) == 0, "setup");
  unlink(ctl.c_str());
  spit(ctl, "x");  // a regular file in the way
  bindfx::make_links(pairs);
  CHECK(link_target(gpu) == "/dev/dri/renderD128" && link_target(ctl) == "/dev/kfd", "replaced");
  // longer and shorter targets that share a prefix are wrong
  unlink(ctl.c_str());
  CHECK(symlink("/dev/kfd2", ctl.c_str()) == 0, "setup");
  bindfx::make_links(pairs);
  CHECK(link_target(ctl) == "/dev/kfd", "longer target");
  unlink(ctl.c_str());
  CHECK(symlink("/dev/kf", ctl.c_str()) == 0, "setup");
  bindfx::make_links(pairs);
  CHECK(link_target(ctl) == "/dev/kfd", "shorter target");
  // a missing directory is ENOENT, a directory in the way cannot be unlinked
  CHECK(err_of([](const std::string& p) { bindfx::force_symlink("/dev/kfd", p); },
               root + "/gone/link") == ENOENT, "ENOENT");
  mkdir((root + "/dir").c_str(), 0700);
  int e = err_of([](const std::string& p) { bindfx::force_symlink("/dev/kfd", p); }, root + "/dir");
  CHECK(e == EISDIR || e == EPERM, "directory in the way");
  rmdir((root + "/dir").c_str());
  bindfx::unlink_many({gpu, ctl});
  CHECK(listing(root).empty(), "links gone");
}

void test_atomic_write() {
  const std::string path = root + "/abcd1234.json";
  const std::string data = "{\"version\": 1, \"gpu_indexes\": [0]}";
  bindfx::atomic_write(path, data.data(), data.size());
  CHECK(slurp(path) == data, "content");
  struct stat st;
  stat(path.c_str(), &st);
  CHECK((st.st_mode & 07777) == 0600, "mode");
  bindfx::atomic_write(path, "", 0);
  CHECK(slurp(path).empty(), "empty payload replaces");
  std::string big(3 << 20, 'x');  // several write() calls' worth on a pipe-like fs
  bindfx::atomic_write(path, big.data(), big.size());
  CHECK(slurp(path) == big, "large payload");
  CHECK(listing(root).size() == 1, "no temp left");
  // failures: the parent is a file (open fails), the target is a non-empty
  // directory (rename fails after the temp was written)
  int e = err_of([](const std::string& p) { bindfx::atomic_write(p, "{}", 2); }, path + "/x.json");
  CHECK(e == ENOTDIR, "ENOTDIR");
  mkdir((root + "/d.json").c_str(), 0700);
  mkdir((root + "/d.json/sub").c_str(), 0700);
  e = err_of([](const std::string& p) { bindfx::atomic_write(p, "{}", 2); }, root + "/d.json");
  CHECK(e == EISDIR || e == ENOTEMPTY || e == EEXIST, "rename onto a directory");
  CHECK(listing(root).size() == 2, "no temp left after a failure");
  rmdir((root + "/d.json/sub").c_str());
  rmdir((root + "/d.json").c_str());
  // 8 threads x 50 writes to one path: one whole payload, no temp file
  std::vector<std::string> payloads;
  for (int t = 0; t < 8; ++t) payloads.push_back(std::string(200 + 37 * t, (char)('a' + t)));
  std::vector<std::thread> threads;
  for (int t = 0; t < 8; ++t)
    threads.emplace_back([t, &payloads, &path] {
      try {
        for (int i = 0; i < 50; ++i)
          bindfx::atomic_write(path, payloads[t].data(), payloads[t].size());
      } catch (const bindfx::SysError& err) {
        CHECK(false, err.what());
      }
    });
  for (auto& th : threads) th.join();
  const std::string got = slurp(path);
  bool whole = false;
  for (auto& p : payloads) whole = whole || got == p;
  CHECK(whole, "one whole payload");
  CHECK(listing(root).size() == 1, "no temp left after the threads");
  bindfx::unlink_many({path});
}

void test_unlink_many() {
  std::vector<std::string> paths;
  for (int i = 0; i < 4; ++i) {
    paths.push_back(root + "/f" + std::to_string(i));
    spit(paths.back(), "x");
  }
  paths.insert(paths.begin() + 1, root + "/missing");
  paths.push_back(root + "/nodir/missing");
  spit(root + "/keep", "k");
  bindfx::unlink_many(paths);
  CHECK(listing(root).size() == 1, "all but keep");
  bindfx::unlink_many(paths);  // all missing
  bindfx::unlink_many({});
  // the first error other than ENOENT is thrown after the rest were tried
  mkdir((root + "/d").c_str(), 0700);
  spit(root + "/after", "x");
  int e = 0;
  std::string where;
  try {
    bindfx::unlink_many({root + "/d", root + "/after", root + "/keep/x"});
  } catch (const bindfx::SysError& err) {
    e = err.err;
    where = err.path;
  }
  CHECK((e == EISDIR || e == EPERM) && where == root + "/d", "first error");
  CHECK(listing(root).size() == 2, "the rest were tried");
  rmdir((root + "/d").c_str());
  bindfx::unlink_many({root + "/keep"});
}

}  // namespace

int main() {
  const char* base = getenv("TMPDIR");
  std::string tmpl = std::string(base && *base ? base : "/tmp") + "/egpu-bindfx-XXXXXX";
  if (!mkdtemp(&tmpl[0])) {
    perror("mkdtemp");
    return 2;
  }
  root = tmpl;
  test_links();
  test_atomic_write();
  test_unlink_many();
  CHECK(listing(root).empty(), "left something behind");
  for (auto& n : listing(root)) unlink((root + "/" + n).c_str());
  rmdir(root.c_str());
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures.load());
    return 1;
  }
  printf("bindfx_selftest OK\n");
  return 0;
}
