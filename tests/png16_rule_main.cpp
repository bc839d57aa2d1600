// The 16-bit PNG rule's host encoder alone (csrc/png16_host.hpp over png16_rule.hpp) as a host program,
// for a sanitizer build:
//   png16_rule_main MANIFEST
// MANIFEST holds one "path n h w" a line, path a file of n * h * w uint16 in native byte order.  For
// each frame the program prints "size hash stats-hash": the file's bytes, their FNV-1a hash (64 bits)
// and the hash of the frame's band statistics (nine int32 a band).  Buffers are sized exactly -- the
// frame by itself, the file at the rule's bound -- so that a sanitizer sees any byte read or written
// past what a call is given.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "../monkey-pose_amd/csrc/png16_host.hpp"

static uint64_t fnv(const void* p, size_t n) {
  uint64_t hash = 1469598103934665603ull;
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n; ++i) hash = (hash ^ b[i]) * 1099511628211ull;
  return hash;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream man(argv[1]);
  std::string line;
  while (std::getline(man, line)) {
    std::istringstream is(line);
    std::string path;
    int n, h, w;
    if (!(is >> path >> n >> h >> w)) return 2;
    std::ifstream f(path, std::ios::binary);
    if (!f) return 2;
    std::vector<char> tmp((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t frame_bytes = (size_t)h * w * 2;
    if (tmp.size() != (size_t)n * frame_bytes) return 2;
    const size_t bound = (size_t)mppng16::bound(h, w);
    const int nb = mppng16::band_count(h, w);
    for (int i = 0; i < n; ++i) {
      // heap copies of the exact size: no slack after the frame, the file or the statistics
      uint16_t* frame = static_cast<uint16_t*>(std::malloc(frame_bytes));
      std::memcpy(frame, tmp.data() + (size_t)i * frame_bytes, frame_bytes);
      uint8_t* file = static_cast<uint8_t*>(std::malloc(bound));
      mppng16h::BandStats* st = static_cast<mppng16h::BandStats*>(std::malloc((size_t)nb * sizeof(mppng16h::BandStats)));
      const size_t size = mppng16h::encode_image(frame, h, w, file, st);
      if (size > bound) return 3;
      std::printf("%zu %016llx %016llx\n", size, (unsigned long long)fnv(file, size),
                  (unsigned long long)fnv(st, (size_t)nb * sizeof(mppng16h::BandStats)));
      std::free(frame), std::free(file), std::free(st);
    }
  }
  return 0;
}
