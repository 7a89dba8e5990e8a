// Stand-alone check of csrc/capi_guard.h (tests/test_capi_guard_native.py builds it with
// -fsanitize=address,undefined and runs it as a child process): guarded, guarded_new, MappedFile.
// argv[1] is an empty directory the program may write into. Prints "ok" and exits 0, or prints the
// failed check and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../nzcb-circom_amd/csrc/capi_guard.h"

using namespace nzcb;

static int g_failed = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      g_failed++;                                                 \
    }                                                             \
  } while (0)

struct Thing {
  std::vector<int> v = std::vector<int>(100, 7);  // heap memory a leak check would see
};

static void write_file(const std::string& path, const char* bytes, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(bytes, 1, n, f) != n) {
    std::printf("cannot write %s\n", path.c_str());
    std::exit(2);
  }
  std::fclose(f);
}

static nzcb_err preset() {
  nzcb_err e;
  e.code = 77;
  std::snprintf(e.msg, sizeof(e.msg), "%s", "left over");
  return e;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];

  // guarded: success clears a pre-set code and leaves the message alone
  {
    nzcb_err e = preset();
    bool ran = false;
    CHECK(guarded(&e, [&] { ran = true; }) == 0);
    CHECK(ran && e.code == 0 && std::strcmp(e.msg, "left over") == 0);
  }
  // guarded: an Error keeps its code and text
  {
    nzcb_err e = preset();
    CHECK(guarded(&e, [] { throw Error(NZCB_ERR_FORMAT, "x"); }) == NZCB_ERR_FORMAT);
    CHECK(e.code == NZCB_ERR_FORMAT && std::strcmp(e.msg, "x") == 0);
  }
  // guarded: any other exception is NZCB_ERR_INTERNAL with its what()
  {
    nzcb_err e = preset();
    CHECK(guarded(&e, [] { throw std::runtime_error("y"); }) == NZCB_ERR_INTERNAL);
    CHECK(e.code == NZCB_ERR_INTERNAL && std::strcmp(e.msg, "y") == 0);
  }
  // guarded: a message longer than err.msg is cut and NUL-terminated
  {
    nzcb_err e = preset();
    const std::string big(4 * sizeof(e.msg), 'm');
    CHECK(guarded(&e, [&] { throw Error(NZCB_ERR_ARG, big); }) == NZCB_ERR_ARG);
    CHECK(e.msg[sizeof(e.msg) - 1] == 0);
    CHECK(std::strlen(e.msg) == sizeof(e.msg) - 1);
    CHECK(std::string(e.msg) == big.substr(0, sizeof(e.msg) - 1));
  }
  // guarded: a NULL err on every path
  CHECK(guarded(nullptr, [] {}) == 0);
  CHECK(guarded(nullptr, [] { throw Error(NZCB_ERR_HIP, "h"); }) == NZCB_ERR_HIP);
  CHECK(guarded(nullptr, [] { throw std::logic_error("l"); }) == NZCB_ERR_INTERNAL);

  // guarded_new: the object on success, NULL and no leak when f throws after building it
  {
    nzcb_err e = preset();
    Thing* t = guarded_new<Thing>(&e, [] { return std::make_unique<Thing>(); });
    CHECK(t && t->v.size() == 100 && t->v[99] == 7);
    CHECK(e.code == 0 && std::strcmp(e.msg, "left over") == 0);
    delete t;
  }
  {
    nzcb_err e = preset();
    Thing* t = guarded_new<Thing>(&e, [] {
      auto made = std::make_unique<Thing>();
      if (made->v.size() == 100) throw Error(NZCB_ERR_ARG, "late");
      return made;
    });
    CHECK(t == nullptr && e.code == NZCB_ERR_ARG && std::strcmp(e.msg, "late") == 0);
    CHECK(guarded_new<Thing>(nullptr, []() -> std::unique_ptr<Thing> { throw std::runtime_error("z"); }) == nullptr);
    Thing* u = guarded_new<Thing>(nullptr, [] { return std::make_unique<Thing>(); });
    CHECK(u != nullptr);
    delete u;
  }

  // MappedFile
  {
    const std::string missing = dir + "/missing.bin";
    nzcb_err e = preset();
    CHECK(guarded(&e, [&] { MappedFile f(missing.c_str(), "the thing", "thing is empty"); }) == NZCB_ERR_ARG);
    CHECK(std::string(e.msg) == "cannot open " + missing);
  }
  {
    const std::string empty = dir + "/empty.bin";
    write_file(empty, "", 0);
    nzcb_err e = preset();
    CHECK(guarded(&e, [&] { MappedFile f(empty.c_str(), "the thing", "thing is empty"); }) == NZCB_ERR_FORMAT);
    CHECK(std::strcmp(e.msg, "thing is empty") == 0);
  }
  {
    const std::string three = dir + "/three.bin";
    write_file(three, "abc", 3);
    nzcb_err e = preset();
    std::string got;
    CHECK(guarded(&e, [&] {
            MappedFile f(three.c_str(), "the thing", "thing is empty");
            got.assign(reinterpret_cast<const char*>(f.data), f.size);
          }) == 0);
    CHECK(got == "abc" && e.code == 0);
  }

  if (g_failed) return 1;
  std::printf("ok\n");
  return 0;
}
