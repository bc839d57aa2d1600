// The decoder's rule alone (csrc/pngdec_rule.hpp) as a host program, for a sanitizer build:
//   pngdec_rule_main MANIFEST
// MANIFEST holds one "path h w format" a line; for each the program prints "status hash", the hash
// (FNV-1a, 64 bits) over the decoded image.  Buffers are sized exactly, so that a sanitizer sees any
// byte read or written past what a call is given.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "../monkey-pose_amd/csrc/pngdec_rule.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream man(argv[1]);
  std::string line;
  while (std::getline(man, line)) {
    std::istringstream is(line);
    std::string path;
    int h, w, format;
    if (!(is >> path >> h >> w >> format)) return 2;
    std::ifstream f(path, std::ios::binary);
    if (!f) return 2;
    // heap copies of the exact size: no slack after the file
    std::vector<char> tmp((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int64_t size = (int64_t)tmp.size();
    uint8_t* file = static_cast<uint8_t*>(std::malloc(size ? size : 1));
    for (int64_t i = 0; i < size; ++i) file[i] = (uint8_t)tmp[i];
    uint8_t* z = static_cast<uint8_t*>(std::malloc(size ? size : 1));
    const int64_t rawn = mppd::raw_bytes(h, w, format), outn = (int64_t)h * mppd::row_bytes(w, format);
    uint8_t* raw = static_cast<uint8_t*>(std::malloc(rawn));
    uint16_t* out = static_cast<uint16_t*>(std::malloc(outn + 1));
    const int st = mppd::decode_file_host(file, size, h, w, format, z, raw, out);
    uint64_t hash = 1469598103934665603ull;
    const uint8_t* o = reinterpret_cast<const uint8_t*>(out);
    for (int64_t i = 0; i < outn; ++i) hash = (hash ^ o[i]) * 1099511628211ull;
    std::printf("%d %016llx\n", st, (unsigned long long)hash);
    std::free(file), std::free(z), std::free(raw), std::free(out);
  }
  return 0;
}
