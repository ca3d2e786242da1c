// fuzz_sequence.cc -- sanitizer harness for the sequence walk (libjxl_amd/csrc/sequence_walk.h: ParseImagePart and
// WalkSequence, the code jxlhip_codestream_sequence_info and jxlhip_decode_codestream_next run, with
// libjxl_amd/csrc/entropy.cc compiled INTO this binary with -fsanitize=address,undefined): for every codestream given,
// the walk -- image header, then per frame the frame header (durations, crops and blending info are read), the TOC, the
// skip over the sections, the save analysis and the counters -- on an exact-size heap block: undamaged first, then
// truncated at every byte and with every single bit flipped.  Walk errors are the expected outcome; any out-of-bounds
// access or undefined behaviour ends the program.  Prints "<ok> <rejected>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../libjxl_amd/csrc/sequence_walk.h"

namespace {
typedef std::vector<uint8_t> Bytes;

// the number of frames walked, 0 = refused
unsigned Walk(const uint8_t* d, size_t len) {
  uint8_t* p = (uint8_t*)malloc(len ? len : 1);  // exact size: one byte past the end is an ASAN report
  if (len) memcpy(p, d, len);
  jxlhip::Sequence s;
  const int rc = jxlhip::WalkSequence(p, len, &s);
  unsigned frames = 0;
  if (rc == JXLHIP_OK) {
    frames = (unsigned)s.frames.size();
    // what the decode call relies on: the frames lie inside the file, in order, and the last one is the last
    size_t at = 0;
    for (const jxlhip::SeqFrame& f : s.frames) {
      if (f.header_bit < at || f.toc_bit < f.header_bit || f.end_bit < f.toc_bit || f.end_bit > len * 8 || f.end_bit % 8) abort();
      at = f.end_bit;
    }
    if (!frames || !s.frames.back().fh.is_last || s.displayed == 0) abort();
  }
  free(p);
  return frames;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  unsigned long long ok = 0, rejected = 0;
  for (int i = 1; i < argc; i++) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) return 2;
    Bytes cs;
    uint8_t buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) cs.insert(cs.end(), buf, buf + k);
    fclose(f);
    if (Walk(cs.data(), cs.size()) < 2) {
      fprintf(stderr, "undamaged codestream %s does not walk as a sequence\n", argv[i]);
      return 1;
    }
    for (size_t n = 0; n < cs.size(); n++) {
      if (Walk(cs.data(), n)) {  // a cut file never walks to its last frame
        fprintf(stderr, "%s cut at %zu walks\n", argv[i], n);
        return 1;
      }
      rejected++;
    }
    for (size_t bit = 0; bit < cs.size() * 8; bit++) {
      Bytes b = cs;
      b[bit / 8] ^= (uint8_t)(1u << (bit % 8));
      (Walk(b.data(), b.size()) ? ok : rejected)++;
    }
  }
  printf("%llu %llu\n", ok, rejected);
  return 0;
}
