// The host-only plans of libjxl_amd/csrc/codestream_plan.h -- the container walk (ExtractCodestream through
// CodestreamBytes::Open, whole and partial) and the ticket order of the single runner call (PlanTickets) -- against
// restatements written here.  A stand-alone program, built with -fsanitize=address,undefined by
// tests/test_codestream_plan.py.  Prints "<container inputs run> <ticket lists checked>".
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../libjxl_amd/csrc/codestream_plan.h"

using jxlhip::CodestreamBytes;
typedef std::vector<uint8_t> Bytes;

static long g_inputs = 0, g_lists = 0;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, what); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t Rand(uint32_t n) {  // [0, n), xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

// ---- container

static void Put32(Bytes* b, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) b->push_back((uint8_t)(v >> s));
}
static void Append(Bytes* b, const Bytes& more) { b->insert(b->end(), more.begin(), more.end()); }
// how a box states its size: 32 bits, 64 bits (size field 1), or 0 = to the end of the file
enum BoxSize { kSize32, kSize64, kSizeToEnd };
static Bytes Box(const char* type, const Bytes& payload, BoxSize how = kSize32) {
  Bytes b;
  Put32(&b, how == kSize32 ? 8 + (uint32_t)payload.size() : how == kSize64 ? 1 : 0);
  b.insert(b.end(), type, type + 4);
  if (how == kSize64) Put32(&b, 0), Put32(&b, 16 + (uint32_t)payload.size());
  Append(&b, payload);
  return b;
}
static Bytes Jxlp(uint32_t index, const Bytes& part) {
  Bytes p;
  Put32(&p, index);
  Append(&p, part);
  return Box("jxlp", p);
}
static Bytes File(std::initializer_list<Bytes> boxes) {
  static const uint8_t kSig[12] = {0, 0, 0, 0xC, 'J', 'X', 'L', ' ', 0xD, 0xA, 0x87, 0xA};
  Bytes f(kSig, kSig + 12);
  Append(&f, Box("ftyp", Bytes{'j', 'x', 'l', ' ', 0, 0, 0, 0, 'j', 'x', 'l', ' '}));
  for (const Bytes& b : boxes) Append(&f, b);
  return f;
}

// The restatement, for files whose boxes are whole: the jxlc payload, or the jxlp payloads in index order; a duplicate
// or missing index, a second jxlc and a jxlp after a jxlc are refused.
static int Restate(const Bytes& f, Bytes* out) {
  out->clear();
  if (f.size() >= 2 && f[0] == 0xFF && f[1] == 0x0A) return *out = f, JXLHIP_OK;
  std::vector<std::pair<uint32_t, Bytes>> parts;
  int jxlc = 0;
  for (size_t pos = 12; pos < f.size();) {
    uint64_t box = ((uint64_t)f[pos] << 24) | (f[pos + 1] << 16) | (f[pos + 2] << 8) | f[pos + 3];
    size_t header = 8;
    if (box == 1) {
      box = 0, header = 16;
      for (int i = 8; i < 16; i++) box = (box << 8) | f[pos + i];
    }
    const size_t end = box == 0 ? f.size() : pos + (size_t)box;
    const std::string type(f.begin() + pos + 4, f.begin() + pos + 8);
    if (type == "jxlc") {
      if (jxlc++) return JXLHIP_ERR_BAD_STREAM;
      parts.push_back({0u, Bytes(f.begin() + pos + header, f.begin() + end)});
    } else if (type == "jxlp") {
      if (jxlc) return JXLHIP_ERR_BAD_STREAM;
      const uint32_t idx = ((uint32_t)f[pos + header] << 24) | (f[pos + header + 1] << 16) | (f[pos + header + 2] << 8) | f[pos + header + 3];
      parts.push_back({idx & 0x7FFFFFFFu, Bytes(f.begin() + pos + header + 4, f.begin() + end)});
    }
    pos = end;
  }
  std::stable_sort(parts.begin(), parts.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  for (size_t i = 0; i < parts.size(); i++) {
    if (parts[i].first != i) return JXLHIP_ERR_BAD_STREAM;
    Append(out, parts[i].second);
  }
  return parts.empty() ? JXLHIP_ERR_BAD_STREAM : JXLHIP_OK;
}

// Open on an exact-size heap block (a read past the input is a sanitizer report); every byte handed out is read
static int Open(const uint8_t* data, size_t size, bool partial, Bytes* got) {
  uint8_t* block = (uint8_t*)malloc(size ? size : 1);
  if (size) memcpy(block, data, size);
  CodestreamBytes b;
  const int rc = b.Open(block, size, partial);
  got->clear();
  if (rc == JXLHIP_OK) got->assign(b.cs, b.cs + b.n);
  free(block);
  g_inputs++;
  return rc;
}

static void CheckContainer(const char* what, const Bytes& f, const Bytes& payload, bool prefix_rule) {
  Bytes want, got;
  const int rc = Restate(f, &want);
  CHECK(rc != JXLHIP_OK || want == payload);
  for (int partial = 0; partial < 2; partial++) {
    const int orc = Open(f.data(), f.size(), partial != 0, &got);
    // (a file without any codestream box, read as a partial file, waits for more input)
    CHECK(orc == rc || (partial && rc != JXLHIP_OK && orc == JXLHIP_ERR_NEED_MORE_INPUT));
    CHECK(rc != JXLHIP_OK || got == want);
    // damage: errors are the expected outcome, a sanitizer report ends the program
    for (size_t n = 0; n < f.size(); n++) {
      const int prc = Open(f.data(), n, partial != 0, &got);
      if (!partial || !prefix_rule) continue;
      // a proper prefix of a valid file, read as a partial file: more input needed, or a prefix of the payload
      CHECK(prc == JXLHIP_ERR_NEED_MORE_INPUT || prc == JXLHIP_OK);
      CHECK(prc != JXLHIP_OK || (got.size() <= payload.size() && std::equal(got.begin(), got.end(), payload.begin())));
    }
    for (size_t bit = 0; bit < 8 * std::min<size_t>(64, f.size()); bit++) {
      Bytes d = f;
      d[bit / 8] ^= (uint8_t)(1u << (bit % 8));
      Open(d.data(), d.size(), partial != 0, &got);
    }
  }
}

static void Containers() {
  Bytes payload = {0xFF, 0x0A};
  for (int i = 0; i < 201; i++) payload.push_back((uint8_t)Rand(256));
  const Bytes a(payload.begin(), payload.begin() + 90), b(payload.begin() + 90, payload.end());
  const uint32_t kLast = 0x80000000u;
  CheckContainer("a bare codestream", payload, payload, true);
  CheckContainer("one jxlc box", File({Box("jxlc", payload)}), payload, true);
  CheckContainer("two jxlp boxes", File({Jxlp(0, a), Jxlp(1 | kLast, b)}), payload, true);
  // (read as a partial file, a prefix that holds the box of index 1 alone is refused, and one that ends inside the box
  // of index 0 gives that box's bytes with the whole of index 1 behind them: no prefix of the payload)
  CheckContainer("two jxlp boxes, swapped", File({Jxlp(1 | kLast, b), Jxlp(0, a)}), payload, false);
  CheckContainer("a 64-bit box size", File({Box("jxlc", payload, kSize64)}), payload, true);
  CheckContainer("a box of size 0", File({Box("jxlc", payload, kSizeToEnd)}), payload, true);
  CheckContainer("a foreign box in between", File({Jxlp(0, a), Box("Exif", Bytes(12, 0)), Jxlp(1 | kLast, b)}), payload, true);
  // what the restatement refuses, the walk refuses
  const char* what = "refused files";
  Bytes none;
  for (const Bytes& f : {File({Jxlp(0, a), Jxlp(0 | kLast, b)}), File({Jxlp(0, a), Jxlp(2 | kLast, b)}), File({Jxlp(1 | kLast, b)}),
                         File({Box("jxlc", a), Box("jxlc", b)}), File({Box("jxlc", a), Jxlp(0 | kLast, b)}), File({})}) {
    CHECK(Restate(f, &none) == JXLHIP_ERR_BAD_STREAM);
    CheckContainer(what, f, payload, false);
  }
}

// ---- ticket order

struct Frame {
  uint32_t xsg, ysg;  // AC groups (256 x 256 pixels) across and down
};

static void CheckTickets(const Frame& fr, uint32_t np, const std::vector<size_t>& dsz, const std::vector<size_t>& asz) {
  const char* what = "ticket order";
  const uint32_t xsize = fr.xsg * 256 - 100, xsb = (xsize + 7) / 8, gd = 256;  // (a DC group: 256 x 256 blocks)
  const uint32_t xdg = (fr.xsg + 7) / 8, ndc = xdg * ((fr.ysg + 7) / 8), ng = fr.xsg * fr.ysg;
  std::vector<uint32_t> dc_order(3, 77u);
  std::vector<std::vector<uint32_t>> ac_of_dc(2, std::vector<uint32_t>(5, 9u));  // (whatever an earlier frame left)
  uint32_t stray = 0;
  CHECK(jxlhip::PlanTickets(ndc, ng, np, dsz.data(), asz.data(), xsize, xsb, gd, &dc_order, &ac_of_dc, &stray));
  // the restatement: (bytes, index) pairs, stable-sorted by descending bytes (a size from 2^32 on counts as 2^32 - 1) ...
  auto sorted = [](std::vector<std::pair<uint64_t, uint32_t>> v) {
    for (auto& q : v) q.first = std::min<uint64_t>(q.first, 0xFFFFFFFFull);
    std::stable_sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    return v;
  };
  std::vector<std::pair<uint64_t, uint32_t>> dc(ndc), ac(ng);
  for (uint32_t g = 0; g < ndc; g++) dc[g] = {dsz[g], g};
  for (uint32_t g = 0; g < ng; g++) {
    uint64_t bytes = 0;
    for (uint32_t p = 0; p < np; p++) bytes += asz[(size_t)p * ng + g];
    ac[g] = {bytes, g};
  }
  dc = sorted(dc), ac = sorted(ac);
  CHECK(dc_order.size() == ndc + 1 && dc_order[0] == ndc);
  for (uint32_t i = 0; i < ndc; i++) CHECK(dc_order[i + 1] == dc[i].second);
  // ... and the AC groups of DC group d: a scan of the sorted list for the groups of its 8 x 8 rectangle
  CHECK(ac_of_dc.size() == ndc);
  std::vector<uint32_t> seen(ng, 0);
  for (uint32_t d = 0; d < ndc; d++) {
    std::vector<uint32_t> want;
    for (const auto& q : ac)
      if ((q.second % fr.xsg) / 8 == d % xdg && (q.second / fr.xsg) / 8 == d / xdg) want.push_back(q.second);
    CHECK(ac_of_dc[d] == want);
    for (uint32_t g : ac_of_dc[d]) seen[g]++;
  }
  for (uint32_t g = 0; g < ng; g++) CHECK(seen[g] == 1);
  std::vector<uint32_t> perm(dc_order);
  std::sort(perm.begin(), perm.end());
  for (uint32_t i = 0; i <= ndc; i++) CHECK(perm[i] == i);
  // fewer DC groups than the AC groups lie under: refused, naming one of them
  if (ndc > 1) {
    CHECK(!jxlhip::PlanTickets(ndc - 1, ng, np, dsz.data(), asz.data(), xsize, xsb, gd, &dc_order, &ac_of_dc, &stray));
    CHECK(stray < ng && ((stray / fr.xsg) / 8) * xdg + (stray % fr.xsg) / 8 == ndc - 1);
  }
  g_lists++;
}

static void Tickets() {
  static const Frame kFrames[4] = {{1, 1}, {8, 8}, {9, 8}, {17, 9}};
  for (const Frame& fr : kFrames) {
    const uint32_t ndc = ((fr.xsg + 7) / 8) * ((fr.ysg + 7) / 8), ng = fr.xsg * fr.ysg;
    for (uint32_t np = 1; np <= 3; np++) {
      // ties: all sizes equal; sizes at and above 2^32, which the key clamps
      std::vector<size_t> dsz(ndc, 1000), asz((size_t)np * ng, 50);
      CheckTickets(fr, np, dsz, asz);
      dsz[ndc - 1] = (size_t)1 << 32, dsz[0] = ((size_t)1 << 32) + 5;
      asz[ng - 1] = (size_t)1 << 32, asz[ng / 2] = ((size_t)1 << 33) + 1, asz[(size_t)(np - 1) * ng] = 0xFFFFFFFFu;
      CheckTickets(fr, np, dsz, asz);
    }
    for (int it = 0; it < 300; it++) {
      const uint32_t np = 1 + it % 3, range = it % 2 ? 7 : 200000;  // (half the lists: a handful of values, ties everywhere)
      std::vector<size_t> dsz(ndc), asz((size_t)np * ng);
      for (size_t& s : dsz) s = Rand(range);
      for (size_t& s : asz) s = Rand(range);
      CheckTickets(fr, np, dsz, asz);
    }
  }
}

int main() {
  Containers();
  Tickets();
  printf("%ld %ld\n", g_inputs, g_lists);
  return 0;
}
