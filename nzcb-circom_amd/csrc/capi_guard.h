// The C-ABI boundary, host side only (no HIP header): the exception every layer below throws,
// the one place where exceptions become nzcb_err codes, and the read-only file mapping of the
// *_file entry points.
//
// The error contract (include/nzcb.h, next to nzcb_err): an entry point that takes an nzcb_err*
// sets err->code on every return, 0 on success, and writes err->msg only on failure.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../include/nzcb.h"

namespace nzcb {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// Error codes: NZCB_* from include/nzcb.h. Fills `err` (may be NULL).
inline void set_err(nzcb_err* err, int code, const char* msg) {
  if (!err) return;
  err->code = code;
  std::snprintf(err->msg, sizeof(err->msg), "%s", msg);
}

// The body of an int-returning entry point: 0, or the code of what `f` threw.
template <class F>
int guarded(nzcb_err* err, F&& f) {
  try {
    f();
    if (err) err->code = 0;
    return 0;
  } catch (const Error& e) {
    set_err(err, e.code, e.what());
    return e.code;
  } catch (const std::exception& e) {
    set_err(err, NZCB_ERR_INTERNAL, e.what());
    return NZCB_ERR_INTERNAL;
  }
}

// The body of a handle-returning entry point: `f` returns the new object as a std::unique_ptr<T>
// (whatever it built before it threw is then freed by its own unwinding); NULL on failure.
template <class T, class F>
T* guarded_new(nzcb_err* err, F&& f) {
  T* out = nullptr;
  guarded(err, [&] { out = std::unique_ptr<T>(f()).release(); });
  return out;
}

// A file mapped read-only for the duration of a call. `what` names it in the mmap failure
// ("mmap of <what> failed"), `empty_msg` is the NZCB_ERR_FORMAT text for a file of no bytes.
struct MappedFile {
  const uint8_t* data = nullptr;
  size_t size = 0;
  MappedFile(const char* path, const char* what, const char* empty_msg) {
    const int fd = open(path, O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0) {
      if (fd >= 0) close(fd);
      throw Error(NZCB_ERR_ARG, std::string("cannot open ") + path);
    }
    if (st.st_size == 0) {
      close(fd);
      throw Error(NZCB_ERR_FORMAT, empty_msg);
    }
    void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) throw Error(NZCB_ERR_INTERNAL, std::string("mmap of ") + what + " failed");
    data = static_cast<const uint8_t*>(m);
    size = (size_t)st.st_size;
  }
  ~MappedFile() { munmap(const_cast<uint8_t*>(data), size); }
  MappedFile(const MappedFile&) = delete;
  MappedFile& operator=(const MappedFile&) = delete;
};

}  // namespace nzcb
