// error.hpp -- the engine's exception and its argument check.  Plain C++: the host-only headers (load_host.hpp) throw it too.
#pragma once
#include <stdexcept>
#include <string>

#include "../../include/katana_hip.h"

namespace ktn {

struct Error : public std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define KTN_REQUIRE(cond, msg)                                   \
    do {                                                         \
        if (!(cond)) throw ::ktn::Error(KTN_E_INVALID, (msg));   \
    } while (0)

}  // namespace ktn
