// snapshot_format_check.cpp -- the snapshot format's writer and validating reader on their own, for a build under the host
// sanitizers (tests/test_snapshot_format.py: g++ -fsanitize=address,undefined).  Writes a synthetic blob with the format's writer,
// validates it, every truncation of it, and a copy with each single byte of its head (header, options, scalars, section table)
// altered.  Every outcome must be "ok" or an error text; the sanitizers must have nothing to say.  Needs no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../libcloudphxx_amd/csrc/lcx_snapshot_format.hpp"

using namespace lcx::snap;

int main()
{
  layout L;
  L.real_kind = 4; L.lib_version = "format check";
  L.add_opt("nx", 4); L.add_opt("dt", 0x3ff0000000000000ull); L.add_opt("strict_fp", 1);
  L.add_scalar("n_part", 37); L.add_scalar("n_storage", 41); L.add_scalar("n_cell", 8); L.add_scalar("rng_call", 5);
  L.add_section("n", ELEM_UINT, 8, 41); L.add_section("rw2", ELEM_REAL, 4, 41); L.add_section("cell.th", ELEM_REAL, 4, 8);
  L.add_section("cell.vt_pre", ELEM_BYTES, 12, 8); L.add_section("empty", ELEM_UINT, 4, 0);
  const size_t total = size_t(L.finish());
  // the blob lives in a heap block of exactly its size, so that a read past the end is seen by the address sanitizer
  std::vector<unsigned char> blob(total);
  for (size_t i = size_t(L.data_off); i < total; ++i) blob[i] = (unsigned char)(i * 131 + 7);
  for (section &s : L.sections) s.checksum = checksum64(blob.data() + s.offset, size_t(s.count * s.elem_bytes));
  L.write_head(blob.data());

  view v; std::string err;
  if (!validate(blob.data(), blob.size(), v, err)) { printf("the blob as written does not validate: %s\n", err.c_str()); return 1; }
  if (v.sections.size() != 5 || get_name(v.sections[3].name) != "cell.vt_pre" || v.find(v.scalars, "n_storage")->bits != 41 || !v.find_section("rw2") || v.find_section("no such"))
  { printf("the reader does not return what the writer wrote\n"); return 1; }
  for (const section &s : v.sections)
    if (checksum64(blob.data() + s.offset, size_t(s.count * s.elem_bytes)) != s.checksum) { printf("section checksum lost\n"); return 1; }
  if (describe(v).find("section cell.th: real32 x 8") == std::string::npos) { printf("describe: %s\n", describe(v).c_str()); return 1; }

  size_t n_ok = 0, n_err = 0;
  // every truncation, each in a block of its own size
  for (size_t n = 0; n < total; ++n) {
    std::vector<unsigned char> cut(blob.begin(), blob.begin() + n);
    view w; std::string e;
    if (validate(cut.empty() ? nullptr : cut.data(), cut.size(), w, e)) { printf("a blob cut to %zu of %zu bytes validates\n", n, total); return 1; }
    if (e.find("truncated") == std::string::npos) { printf("cut to %zu bytes: %s\n", n, e.c_str()); return 1; }
    ++n_err;
  }
  // every single byte of the head altered, three ways
  for (size_t i = 0; i < size_t(L.data_off); ++i)
    for (unsigned char x : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xff}) {
      std::vector<unsigned char> bad(blob);
      bad[i] ^= x;
      view w; std::string e;
      if (validate(bad.data(), bad.size(), w, e)) {
        ++n_ok;
        // (an "ok" must still be safe to walk)
        for (const section &s : w.sections) if (s.offset + s.count * s.elem_bytes > bad.size()) { printf("an accepted section overruns the blob\n"); return 1; }
        (void)describe(w);
      }
      else { if (e.empty()) { printf("an error without a text\n"); return 1; } ++n_err; }
    }
  // a byte altered between the head's last block and data_off is padding that the head's checksum covers: nothing altered may pass
  if (n_ok != 0) { printf("%zu altered heads validate\n", n_ok); return 1; }
  // checksum64: the words' positions count, the order of summation does not
  unsigned char w16[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, sw[16];
  memcpy(sw, w16 + 8, 8); memcpy(sw + 8, w16, 8);
  if (checksum64(w16, 16) == checksum64(sw, 16)) { printf("two words swapped leave the checksum unchanged\n"); return 1; }
  if (checksum64(w16, 8) + checksum64(w16 + 8, 8, 1) != checksum64(w16, 16)) { printf("the checksum is not a sum over the words\n"); return 1; }
  if (checksum64(w16, 0) != 0) { printf("the checksum of nothing is not zero\n"); return 1; }
  printf("ok: %zu rejected, %zu accepted\n", n_err, n_ok);
  return 0;
}
