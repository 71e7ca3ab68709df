// <OpenImageDenoise/oidn.hpp> for a program written against OIDN: this library's veneer (csrc/oidn_api.h) and OIDN's namespace macros.
#pragma once
#include "../../oidn_api.h"
#define OIDN_NAMESPACE oidn
#define OIDN_NAMESPACE_BEGIN namespace oidn {
#define OIDN_NAMESPACE_END }
#define OIDN_NAMESPACE_USING using namespace oidn;
