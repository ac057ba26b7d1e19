// pt_entry.cpp -- the checks and the copy the entries share (rule: pt_entry.h).  No context is read here.
#include "pt_entry.h"

int check_plane(const char* who, const char* name, const void* p, uint32_t align, bool may_be_null) {
    if (!p && !may_be_null) return fail(PT_ERR_INVALID_ARG, "%s: %s is null", who, name);
    if ((uintptr_t)p % align) return fail(PT_ERR_INVALID_ARG, "%s: %s must be %u-byte aligned", who, name, align);
    return PT_OK;
}

bool ranges_overlap(const Range& a, const Range& b) {
    if (!a.p || !b.p) return false;
    const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
    return pa < pb + b.bytes && pb < pa + a.bytes;
}

int check_no_alias(const char* who, std::initializer_list<Range> outputs, const Range& input) {
    for (const Range* o = outputs.begin(); o != outputs.end(); ++o) {
        if (ranges_overlap(*o, input)) return fail(PT_ERR_INVALID_ARG, "%s: an output must not alias the samples", who);
        for (const Range* k = o + 1; k != outputs.end(); ++k)
            if (ranges_overlap(*o, *k)) return fail(PT_ERR_INVALID_ARG, "%s: the outputs must not alias one another", who);
    }
    return PT_OK;
}

int check_image_min(const char* who, uint32_t width, uint32_t height) {
    if (width < 2 || height < 2) return fail(PT_ERR_INVALID_ARG, "%s: image %ux%u: width and height must be >= 2", who, width, height);
    return PT_OK;
}

int check_pixel_count(const char* who, uint32_t width, uint32_t height) {
    if ((uint64_t)width * height > (1ull << 30)) return fail(PT_ERR_UNSUPPORTED, "%s: %llu pixels", who, (unsigned long long)width * height);
    return PT_OK;
}

int check_image_size(const char* who, uint32_t width, uint32_t height) {
    if (int rc = check_image_min(who, width, height)) return rc;
    return check_pixel_count(who, width, height);
}

int check_whole_image(const char* who, const char* verb, const char* tail, const PtRenderParams* prm, bool band_index_too) {
    if (prm->band_count > 1 || (band_index_too && prm->band_index != 0))
        return fail(PT_ERR_INVALID_ARG, "%s%s the whole image (band_count = 1)%s", who, verb, tail);
    return PT_OK;
}

int copy_back(std::initializer_list<CopyBack> copies) {
    for (const CopyBack& k : copies)
        if (k.host) HIP_TRY(hipMemcpy(k.host, k.dev, k.bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}
