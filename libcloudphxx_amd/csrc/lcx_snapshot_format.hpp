// lcx_snapshot_format.hpp -- the layout of a snapshot blob (include/lcx_state.h), its writer and its validating reader.
//
// Host code only, no HIP include: lcx_core.hip uses it to write and read a blob, lcx_snapshot_describe validates one without a device,
// and tools/snapshot_format_check.cpp compiles it alone under the host sanitizers.
//
//   [header 256 B][options: n_opts x named value][scalars: n_scalars x named value][section table: n_sections x 64 B][pad to 64 B]
//   [section 0][pad][section 1][pad] ...                                  every section begins at a multiple of 64 bytes
//
// Everything is little-endian, as the devices and hosts this library runs on are.  The reader trusts nothing: every offset and count is
// checked against the bytes it was given before it is used, and the checksum of the head (header + options + scalars + table, with the
// header's own checksum field taken as zero) is compared last, so that a damaged field is named where it can be.
#ifndef LCX_SNAPSHOT_FORMAT_HPP
#define LCX_SNAPSHOT_FORMAT_HPP

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace lcx {
namespace snap {

static const char MAGIC[8] = {'L', 'C', 'X', 'S', 'N', 'A', 'P', '1'};
static const uint32_t FORMAT_VERSION = 1;
static const size_t ALIGN = 64;
static const size_t NAME_LEN = 32;
// the device <-> host copies of a save or a load go through two page-locked chunks of this size (recorded in the header)
static const uint64_t CHUNK_BYTES = 32ull << 20;

enum elem_type : uint32_t { ELEM_UINT = 0, ELEM_REAL = 1, ELEM_BYTES = 2 };

struct header {                 // 256 bytes
  char magic[8];
  uint32_t format_version, header_bytes;
  uint64_t total_bytes;         // of the whole blob
  uint32_t real_kind;           // 4 or 8
  uint32_t n_opts, n_scalars, n_sections;
  uint64_t opts_off, scalars_off, table_off, data_off;      // data_off: where the first section may begin (= the head's length)
  uint64_t chunk_bytes;
  uint64_t head_checksum;       // of bytes [0, data_off) with this field zero
  char lib_version[64];         // lcx_version() of the writer
  char reserved[104];
};
static_assert(sizeof(header) == 256, "the header is 256 bytes");

struct named_value {            // an option of lcx_opts_init_t or a scalar of the object's state
  char name[NAME_LEN];
  uint64_t bits;                // an integer as it is (signed ones sign-extended), a double by its bit pattern
};
static_assert(sizeof(named_value) == 40, "a named value is 40 bytes");

struct section {                // 64 bytes
  char name[NAME_LEN];
  uint32_t elem_type, elem_bytes;
  uint64_t count;               // elements
  uint64_t offset;              // from the start of the blob, a multiple of ALIGN
  uint64_t checksum;            // checksum64 of the count * elem_bytes payload bytes
};
static_assert(sizeof(section) == 64, "a section entry is 64 bytes");

// ---- the checksum: position dependent, independent of the order of summation ----
// sum modulo 2^64, over the 8-byte little-endian words w_i of the data (the tail padded with zeros), of mix(w_i + (i + 1) * GOLDEN);
// mix is the finaliser of splitmix64 (Steele, Lea & Flood 2014).  The device computes the same sum in any order (lcx_snapshot_kernels.hpp: k_checksum64).
static const uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
static inline uint64_t mix64(uint64_t z)
{
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static inline uint64_t checksum64(const void *data, size_t bytes, uint64_t first_word = 0)
{
  const unsigned char *p = static_cast<const unsigned char *>(data);
  uint64_t sum = 0;
  const size_t full = bytes / 8;
  for (size_t i = 0; i < full; ++i) { uint64_t w; memcpy(&w, p + 8 * i, 8); sum += mix64(w + (first_word + i + 1) * GOLDEN); }
  if (bytes % 8) { uint64_t w = 0; memcpy(&w, p + 8 * full, bytes % 8); sum += mix64(w + (first_word + full + 1) * GOLDEN); }
  return sum;
}

static inline size_t align_up(size_t n) { return (n + ALIGN - 1) / ALIGN * ALIGN; }
static inline void set_name(char *dst, const char *src) { memset(dst, 0, NAME_LEN); strncpy(dst, src, NAME_LEN - 1); }
static inline std::string get_name(const char *src) { size_t n = 0; while (n < NAME_LEN && src[n]) ++n; return std::string(src, n); }

// ---- writer: the head of a blob whose sections' counts are known; the payload and the sections' checksums are filled in by the caller ----
struct layout {
  std::vector<named_value> opts, scalars;
  std::vector<section> sections;          // offsets assigned by finish()
  uint32_t real_kind = 8;
  std::string lib_version;
  uint64_t data_off = 0, total_bytes = 0;
  void add_opt(const char *name, uint64_t bits) { named_value v; set_name(v.name, name); v.bits = bits; opts.push_back(v); }
  void add_scalar(const char *name, uint64_t bits) { named_value v; set_name(v.name, name); v.bits = bits; scalars.push_back(v); }
  void add_section(const char *name, uint32_t type, uint32_t elem_bytes, uint64_t count)
  { section s; memset(&s, 0, sizeof s); set_name(s.name, name); s.elem_type = type; s.elem_bytes = elem_bytes; s.count = count; sections.push_back(s); }
  // assigns the offsets; returns the size of the whole blob
  uint64_t finish()
  {
    const uint64_t head = sizeof(header) + (opts.size() + scalars.size()) * sizeof(named_value) + sections.size() * sizeof(section);
    data_off = align_up(head);
    uint64_t at = data_off;
    for (section &s : sections) { s.offset = at; at = align_up(at + s.count * s.elem_bytes); }
    total_bytes = at;
    return total_bytes;
  }
  // writes [0, data_off) into buf (cap >= data_off); call after finish() and after the sections' checksums are known
  void write_head(void *buf) const
  {
    unsigned char *b = static_cast<unsigned char *>(buf);
    memset(b, 0, data_off);
    header h; memset(&h, 0, sizeof h);
    memcpy(h.magic, MAGIC, 8);
    h.format_version = FORMAT_VERSION; h.header_bytes = sizeof(header); h.total_bytes = total_bytes; h.real_kind = real_kind;
    h.n_opts = uint32_t(opts.size()); h.n_scalars = uint32_t(scalars.size()); h.n_sections = uint32_t(sections.size());
    h.opts_off = sizeof(header); h.scalars_off = h.opts_off + opts.size() * sizeof(named_value);
    h.table_off = h.scalars_off + scalars.size() * sizeof(named_value); h.data_off = data_off; h.chunk_bytes = CHUNK_BYTES;
    strncpy(h.lib_version, lib_version.c_str(), sizeof h.lib_version - 1);
    memcpy(b, &h, sizeof h);
    if (!opts.empty()) memcpy(b + h.opts_off, opts.data(), opts.size() * sizeof(named_value));
    if (!scalars.empty()) memcpy(b + h.scalars_off, scalars.data(), scalars.size() * sizeof(named_value));
    if (!sections.empty()) memcpy(b + h.table_off, sections.data(), sections.size() * sizeof(section));
    const uint64_t sum = checksum64(b, data_off);
    memcpy(b + offsetof(header, head_checksum), &sum, 8);
  }
};

// ---- validating reader ----
struct view {
  header h;
  std::vector<named_value> opts, scalars;
  std::vector<section> sections;
  const named_value *find(const std::vector<named_value> &v, const char *name) const
  { for (const named_value &e : v) if (get_name(e.name) == name) return &e; return nullptr; }
  const section *find_section(const char *name) const
  { for (const section &s : sections) if (get_name(s.name) == name) return &s; return nullptr; }
};

// returns true and fills `out`, or false with the reason in `err`.  Reads nothing beyond buf[0, bytes).
static inline bool validate(const void *buf, size_t bytes, view &out, std::string &err)
{
  const unsigned char *b = static_cast<const unsigned char *>(buf);
  if (!b || bytes < sizeof(header)) {
    err = "libcloudph++: snapshot is truncated (" + std::to_string(bytes) + " bytes, the header alone takes " + std::to_string(sizeof(header)) + ")";
    return false;
  }
  header &h = out.h;
  memcpy(&h, b, sizeof h);
  if (memcmp(h.magic, MAGIC, 8) != 0) { err = "libcloudph++: not a snapshot (wrong magic)"; return false; }
  if (h.format_version != FORMAT_VERSION) {
    err = "libcloudph++: snapshot format version " + std::to_string(h.format_version) + " is unknown to this library (it reads version " + std::to_string(FORMAT_VERSION) + ")";
    return false;
  }
  if (h.total_bytes > bytes) {
    err = "libcloudph++: snapshot is truncated (" + std::to_string(bytes) + " of " + std::to_string(h.total_bytes) + " bytes)";
    return false;
  }
  const uint64_t total = h.total_bytes;
  auto fits = [&](uint64_t off, uint64_t n, uint64_t each, uint64_t limit) { return off <= limit && n <= (limit - off) / each; };
  h.lib_version[sizeof h.lib_version - 1] = 0;
  if (h.header_bytes != sizeof(header) || h.data_off > total || h.data_off % ALIGN || h.data_off < sizeof(header) || (h.real_kind != 4 && h.real_kind != 8) ||
      h.opts_off < sizeof(header) || !fits(h.opts_off, h.n_opts, sizeof(named_value), h.data_off) ||
      h.scalars_off < sizeof(header) || !fits(h.scalars_off, h.n_scalars, sizeof(named_value), h.data_off) ||
      h.table_off < sizeof(header) || !fits(h.table_off, h.n_sections, sizeof(section), h.data_off)) {
    err = "libcloudph++: snapshot header is damaged (a block of the head overruns it)";
    return false;
  }
  out.opts.resize(h.n_opts); out.scalars.resize(h.n_scalars); out.sections.resize(h.n_sections);
  if (h.n_opts) memcpy(out.opts.data(), b + h.opts_off, h.n_opts * sizeof(named_value));
  if (h.n_scalars) memcpy(out.scalars.data(), b + h.scalars_off, h.n_scalars * sizeof(named_value));
  if (h.n_sections) memcpy(out.sections.data(), b + h.table_off, h.n_sections * sizeof(section));
  for (const section &s : out.sections) {
    const bool sane = s.elem_bytes >= 1 && s.elem_bytes <= 4096 && s.elem_type <= ELEM_BYTES;
    if (!sane || s.offset < h.data_off || s.offset % ALIGN || !fits(s.offset, s.count, sane ? s.elem_bytes : 1, total)) {
      err = "libcloudph++: snapshot section '" + get_name(s.name) + "' overruns the blob";
      return false;
    }
  }
  // the head's checksum, with its own field taken as zero
  std::vector<unsigned char> head(b, b + h.data_off);
  memset(head.data() + offsetof(header, head_checksum), 0, 8);
  if (checksum64(head.data(), head.size()) != h.head_checksum) { err = "libcloudph++: snapshot header checksum does not match"; return false; }
  return true;
}

static inline std::string describe(const view &v)
{
  static const char *types[] = {"uint", "real", "bytes"};
  char line[256];
  std::string s;
  snprintf(line, sizeof line, "libcloudph++ snapshot: format %u, written by \"%s\", real kind %u, %llu bytes, chunk %llu bytes\n", v.h.format_version, v.h.lib_version,
           v.h.real_kind, (unsigned long long)v.h.total_bytes, (unsigned long long)v.h.chunk_bytes);
  s += line;
  snprintf(line, sizeof line, "options: %u, scalars: %u, sections: %u\n", v.h.n_opts, v.h.n_scalars, v.h.n_sections);
  s += line;
  for (const char *nm : {"n_part", "n_storage", "n_cell", "rng_call"})
    if (const named_value *e = v.find(v.scalars, nm)) { snprintf(line, sizeof line, "%s = %llu\n", nm, (unsigned long long)e->bits); s += line; }
  for (const section &e : v.sections) {
    snprintf(line, sizeof line, "section %s: %s%u x %llu at %llu, checksum %016llx\n", get_name(e.name).c_str(), types[e.elem_type], e.elem_bytes * 8,
             (unsigned long long)e.count, (unsigned long long)e.offset, (unsigned long long)e.checksum);
    s += line;
  }
  return s;
}

}  // namespace snap
}  // namespace lcx
#endif
