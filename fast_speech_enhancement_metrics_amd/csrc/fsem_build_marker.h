// The build's content hash and offload target as marker strings the host layer reads from the
// built file without loading it (_build.library_build_id, library_build_arch; _build.py passes
// -DFSEM_BUILD_ID and -DFSEM_BUILD_ARCH).  The target is recorded apart from the hash: a library
// built for another target is refused at load rather than rebuilt.  Included by exactly one
// source of each library, which must hold one id and one arch.
#pragma once

#ifndef FSEM_BUILD_ID
#define FSEM_BUILD_ID "unknown"
#endif
#ifndef FSEM_BUILD_ARCH
#define FSEM_BUILD_ARCH "unknown"
#endif

namespace fsem {
constexpr int kBuildIdPrefix = 14;  // strlen("FSEM_BUILD_ID:")
__attribute__((used)) static const char kBuildIdMarker[] = "FSEM_BUILD_ID:" FSEM_BUILD_ID;
__attribute__((used)) static const char kBuildArchMarker[] = "FSEM_BUILD_ARCH:" FSEM_BUILD_ARCH;
}  // namespace fsem
