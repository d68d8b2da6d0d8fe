// bk_codecache.h -- the on-disk cache of compiled code (GPU code objects, host modules): where it is, and what may be loaded from it.
// POSIX and the standard library only; the keys (what a name is derived from) are the callers' business (bk_modules.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bk {
#pragma GCC visibility push(hidden)

uint64_t fnv1a64(const void *data, size_t n, uint64_t h = 1469598103934665603ull);

// Where compiled lens modules are kept: bk_set_cache_dir() if the host called it, else $BLINKY_HIP_CACHE ("" or "off"
// disables the disk cache), else $XDG_CACHE_HOME/blinky_hip, else $HOME/.cache/blinky_hip.
std::string cache_dir();

struct Sha256 {
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    unsigned char buf[64];
    uint64_t len = 0;
    size_t fill = 0;
    void block(const unsigned char *p);
    void update(const void *data, size_t n);
    void update(const std::string &t) { const uint64_t n = t.size(); update(&n, sizeof n); update(t.data(), t.size()); }      // (length-prefixed: "ab","c" != "a","bc")
    void finish(unsigned char out[32]);
};
std::string hex128(Sha256 &s);                                         // the first 128 bits of the digest, in hex
void trailer_of(const void *data, size_t n, unsigned char out[40]);    // "BKSHA256" + the SHA-256 of data

// a directory this user owns, that nobody else can write to and that is no link; made (0700) if it does not exist
bool cache_dir_ok(const std::string &dir, bool create);
// a regular file of this user's that nobody else can write to, opened without following a link; -1 if it is not that
int open_checked(const std::string &path);
// the whole file behind `fd` minus a valid trailer; false if it is short, torn or altered
bool read_verified(int fd, std::vector<char> *out);
bool write_all(int fd, const void *data, size_t n);

// a sealed file (content + trailer) in a directory that passes cache_dir_ok: load is a miss - false - on anything that does not check
// out; store goes through a temporary name and a rename, and does nothing where the directory cannot be trusted or written
bool load_sealed(const std::string &path, std::vector<char> *bytes);
void store_sealed(const std::string &path, const std::vector<char> &bytes);
// append the trailer to a file that is already there (no link) and take it to mode 0600; false if that could not be done
bool seal_in_place(const std::string &path);

#pragma GCC visibility pop
}  // namespace bk
