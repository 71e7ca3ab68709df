// "include/OpenImageDenoise/oidn.hpp", as OIDN's own sources name the header from their root: the same veneer (csrc/oidn_api.h).
#pragma once
#include "../../OpenImageDenoise/oidn.hpp"
