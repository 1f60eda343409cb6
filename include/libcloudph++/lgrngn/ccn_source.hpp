#pragma once   // reference lgrngn/ccn_source.hpp:8 (opts_init.src_type: off, or new super-droplets in the box src_x0 .. src_z1 -- simple: always created, matching: added to existing ones of like size); src_name: ccn_source.hpp:14-18
#include "enum_names.hpp"
namespace libcloudphxx { namespace lgrngn {
  enum class src_t { off, simple, matching };
  const std::unordered_map<src_t, std::string> src_name = detail::enum_names<src_t>({"off", "simple", "matching"});
} }
