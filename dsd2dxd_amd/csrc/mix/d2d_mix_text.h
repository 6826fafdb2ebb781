// d2d_mix_text.h -- the text form of a mix, "g,g,..;g,g,..": what the CLI's --mix takes (mix/d2d_mix_host.cpp)
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace d2d {

// rows separated by ';', decimal gains by ',', every row as long as the first; a gain g becomes round-half-away(g * 32768).  True and the
// rows x cols coefficients (inside mix_check's bounds), or false and the reason.
bool parse_mix_text(const char* text, std::vector<int32_t>& coef, uint32_t& rows, uint32_t& cols, std::string& err);

}  // namespace d2d
