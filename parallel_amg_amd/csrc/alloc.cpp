// alloc.cpp — libpamg's large host buffers on transparent huge pages.
//
// The setup and the uploads of a 512^3 problem allocate tens of GB in std::vector buffers of
// hundreds of MB to several GB each. On 4 KiB pages their cost is dominated by page faults when
// they are first written (the zero fill of a resize, on one thread) and by unmapping when they
// are freed. Buffers of kMinBytes and more are therefore aligned to 2 MiB and marked
// MADV_HUGEPAGE (a hint: where the kernel grants none, nothing changes). Everything is
// malloc-family memory released with free(), exactly as the default operators do, so memory may
// cross freely between code that sees these operators and code that does not.
#include <sys/mman.h>

#include <cstdlib>
#include <new>

namespace {
constexpr std::size_t kHugePage = std::size_t(2) << 20;
constexpr std::size_t kMinBytes = std::size_t(64) << 20;
}  // namespace

void* operator new(std::size_t n) {
    if (n >= kMinBytes) {
        const std::size_t r = (n + kHugePage - 1) & ~(kHugePage - 1);
        if (void* p = std::aligned_alloc(kHugePage, r)) {
            madvise(p, r, MADV_HUGEPAGE);
            return p;
        }
        throw std::bad_alloc();
    }
    if (void* p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void* operator new[](std::size_t n) { return operator new(n); }
void operator delete(void* p) noexcept { std::free(p); }
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }
