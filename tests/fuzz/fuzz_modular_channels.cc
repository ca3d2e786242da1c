// fuzz_modular_channels.cc -- sanitizer harness for the host decode of a lossless (regular Modular) frame of an image with
// extra channels and / or a grey image: tests/fuzz/fuzz_modular_image.cc for jxlhip_modular_image_decode_channels
// (libjxl_amd/csrc/entropy.cc + modular.inc + modular_image.inc compiled INTO this binary with
// -fsanitize=address,undefined).  Damaged copies of genuine files go through jxlhip_image_header_decode ->
// jxlhip_frame_header_decode -> the entry with num_color + num_extra planes, every buffer an exact-size heap block.
//   fuzz_modular_channels <stride> <file> ...
// Per file: the undamaged stream must decode; then byte k is complemented, for k = 0, stride, 2 * stride, ... (stride 1:
// every byte of the file in turn), and every bit of the first 64 bytes is flipped, one at a time.  Prints
// "<ok> <rejected>" over all of them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jxl_hip_entropy.h"
#include "../../include/jxl_hip_frame.h"

namespace {
typedef std::vector<uint8_t> Bytes;

struct Exact {  // an exact-size heap copy: one byte past the end is an ASAN report
  uint8_t* p;
  size_t n;
  Exact(const uint8_t* d, size_t len) : p((uint8_t*)malloc(len ? len : 1)), n(len) {
    if (len) memcpy(p, d, len);
  }
  ~Exact() { free(p); }
};

bool Chain(const Bytes& cs, uint32_t sample_type) {
  Exact all(cs.data(), cs.size());
  jxlhip_image_header ih;
  size_t pos = 0;
  jxlhip_extra_channel extra[4];
  if (jxlhip_image_header_decode(all.p, all.n, &pos, extra, 4, &ih) != JXLHIP_OK) return false;
  if (ih.xyb_encoded || ih.num_extra_channels > 4 || ih.color_encoding.want_icc) return false;
  for (uint32_t e = 0; e < ih.num_extra_channels; e++)  // (what the whole-file calls refuse at the image header)
    if (extra[e].dim_shift != 0 || extra[e].bit_depth.floating_point_sample || extra[e].bit_depth.bits_per_sample == 0 ||
        extra[e].bit_depth.bits_per_sample > 16)
      return false;
  jxlhip_image_info info = {ih.xsize, ih.ysize, ih.xyb_encoded, ih.num_extra_channels, nullptr,
                            ih.have_animation, ih.have_timecodes, 0, ih.bit_depth.bits_per_sample};
  jxlhip_frame_header fh;
  if (jxlhip_frame_header_decode(all.p, all.n, &pos, &info, &fh) != JXLHIP_OK) return false;
  if (fh.num_toc_entries == 0 || fh.num_toc_entries > 4096 || fh.num_groups == 0 || fh.num_groups > 4096) return false;
  if ((uint64_t)fh.xsize * fh.ysize > (1u << 21)) return false;  // bound the fuzzer's allocations
  const size_t ssz = sample_type == JXLHIP_MODULAR_I16 ? 2 : 4;
  const size_t plane = (size_t)fh.xsize * fh.ysize * ssz;
  uint8_t* p[7];
  for (int i = 0; i < 7; i++) p[i] = (uint8_t*)malloc(plane ? plane : 1);
  uint16_t* rct = (uint16_t*)malloc((size_t)fh.num_groups * sizeof(uint16_t));
  jxlhip_modular_image_channels pl;
  memset(&pl, 0, sizeof(pl));
  const jxlhip_color_encoding& ce = ih.color_encoding;
  pl.num_color = !ce.all_default && ce.color_space == JXLHIP_CS_GRAY ? 1 : 3;
  pl.num_extra = ih.num_extra_channels;
  for (uint32_t c = 0; c < pl.num_color; c++) pl.planes[c] = p[c];
  for (uint32_t e = 0; e < pl.num_extra; e++) pl.extra_planes[e] = p[3 + e], pl.extra_bits[e] = extra[e].bit_depth.bits_per_sample;
  pl.stride_samples = fh.xsize;
  pl.sample_type = sample_type;
  pl.group_rct = rct;
  const char* why = nullptr;
  const int rc = jxlhip_modular_image_decode_channels(all.p, all.n, &pos, &fh, nullptr, nullptr, &pl, &why);
  // (a plane that does not fit 16 bits is an answer, and the whole-file call's cue for int32 planes)
  bool ok = rc == JXLHIP_OK || (rc == JXLHIP_ERR_RANGE && sample_type == JXLHIP_MODULAR_I16);
  if (rc == JXLHIP_OK) {  // what the device would be handed: every program within the 42 types, the end inside the bytes
    if (pos > all.n * 8) abort();
    for (uint64_t g = 0; g < fh.num_groups; g++)
      if ((rct[g] & 0xFF) > 41 || (rct[g] >> 8) > 41) abort();
    if ((pl.global_rct & 0xFF) > 41 || (pl.global_rct >> 8) > 41) abort();
    if (pl.num_color == 1 && (pl.global_rct != 0 || pl.groups_on_device != 0)) abort();  // (a grey frame has no programs)
  }
  for (int i = 0; i < 7; i++) free(p[i]);
  free(rct);
  return ok;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const size_t stride = strtoull(argv[1], nullptr, 10);
  if (stride == 0) return 2;
  uint64_t ok = 0, rejected = 0;
  for (int i = 2; i < argc; i++) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) return 2;
    Bytes b;
    uint8_t buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + k);
    fclose(f);
    if (!Chain(b, JXLHIP_MODULAR_I16) || !Chain(b, JXLHIP_MODULAR_I32)) {
      fprintf(stderr, "undamaged codestream %s does not decode\n", argv[i]);
      return 1;
    }
    for (size_t at = 0; at < b.size(); at += stride) {
      Bytes d = b;
      d[at] = (uint8_t)~d[at];
      (Chain(d, (at / stride) & 1 ? JXLHIP_MODULAR_I32 : JXLHIP_MODULAR_I16) ? ok : rejected)++;
    }
    for (size_t bit = 0; bit < 64 * 8 && bit < b.size() * 8; bit++) {
      Bytes d = b;
      d[bit / 8] ^= (uint8_t)(1u << (bit % 8));
      (Chain(d, JXLHIP_MODULAR_I16) ? ok : rejected)++;
    }
  }
  printf("%llu %llu\n", (unsigned long long)ok, (unsigned long long)rejected);
  return 0;
}
