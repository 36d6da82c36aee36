// The FLAC parser of csrc/flac_bits.h -- the text the kernels of csrc/flac.hip compile too -- as a stand-alone host program,
// meant to be built with -fsanitize=address,undefined (tests/test_flac_host.py does): every file named on the command line
// is copied into a heap block of exactly its size, probed and decoded by the sequential twin, and every byte offset of the
// file is offered to the header parser, as the device scan does.  A read outside the block, a signed overflow or a bad shift
// ends the program with the sanitizer's report; a clean run prints one line per file:
//     <file> <probe> <status code> <frames> <samples> <where> <header candidates>
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/flac_sanitize.cpp -o flac_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../beat_this_amd/csrc/flac_bits.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* data = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);   // (exactly n bytes: the sanitizer sees a read of byte n)
    if (n > 0 && fread(data, 1, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    flac::Info in;
    flac::Status st{-1, 0, 0, 0};
    long candidates = 0;
    const int ok = flac::probe(data, n, &in);
    if (ok && in.total_samples < (1ll << 28)) {
      const int64_t ld = (in.total_samples + 3) / 4 * 4;
      std::vector<int32_t> planar((size_t)in.channels * (size_t)ld);
      flac::decode_chain_host(data, in, planar.data(), ld, &st);
      for (int64_t at = in.first_frame; at < n; ++at) {
        flac::Header h;
        if (flac::parse_header(data, n, at, in, h)) {
          flac::NullSink sink;
          flac::walk_frame(data, n, at, in, h, sink, true);
          ++candidates;
        }
      }
    }
    printf("%s %d %d %d %lld %lld %ld\n", argv[a], ok, st.code, st.n_frames, (long long)st.n_samples, (long long)st.where, candidates);
    free(data);
  }
  return 0;
}
