/*
  The C ABI as host_load_test and host_cpu_test_san link it: the functions those programs' links ask for and the locator's entry points (fmi.h), none of which does
  anything.  There is no device behind them: whatever would allocate, upload or download answers BWTM_ENODEV, sizes are 0, handles nullptr.  With
  bwtm_host_alloc failing, HostArray falls back to malloc (support.h).
*/
#include <bwtm.h>

extern "C"
{

const char* bwtm_last_error(void) { return "host_load_test is linked without a device library"; }
int bwtm_host_alloc(uint64_t, void** out) { *out = nullptr; return BWTM_ENODEV; }
void bwtm_host_free(void*) {}
void bwtm_index_free(bwtm_index*) {}
void bwtm_upload_free(bwtm_upload*) {}
uint64_t bwtm_index_bytes(const bwtm_index*) { return 0; }
uint64_t bwtm_index_blocks(const bwtm_index*) { return 0; }
int bwtm_index_encode(bwtm_index*) { return BWTM_ENODEV; }
int bwtm_index_drop_native(bwtm_index*) { return BWTM_ENODEV; }
int bwtm_index_download_data(bwtm_index*, uint8_t*, uint64_t) { return BWTM_ENODEV; }
int bwtm_index_download_samples(bwtm_index*, uint64_t*, uint64_t*) { return BWTM_ENODEV; }
int bwtm_index_samples_width(bwtm_index*, int*) { return BWTM_ENODEV; }
int bwtm_index_download_samples_compact(bwtm_index*, int, void*, uint64_t*) { return BWTM_ENODEV; }
// the Locator of fmi.h
int bwtm_locator_create(const bwtm_index*, uint64_t, bwtm_locator** out) { *out = nullptr; return BWTM_ENODEV; }
void bwtm_locator_free(bwtm_locator*) {}
uint64_t bwtm_locator_bytes(const bwtm_locator*) { return 0; }
int bwtm_locate_batch(const bwtm_locator*, const uint64_t*, uint64_t, uint64_t*, uint64_t*) { return BWTM_ENODEV; }
int bwtm_locate_ranges(const bwtm_locator*, const uint64_t*, const uint64_t*, uint64_t, uint64_t, uint64_t*, uint64_t*, uint64_t*, uint64_t) { return BWTM_ENODEV; }
int bwtm_overlap_batch(const bwtm_locator*, const uint8_t*, const uint64_t*, uint64_t, uint64_t, uint64_t, uint64_t*, uint64_t*, uint64_t*, uint64_t) { return BWTM_ENODEV; }
int bwtm_overlap_sequences(const bwtm_locator*, const uint64_t*, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t*, uint64_t*, uint64_t*, uint64_t) { return BWTM_ENODEV; }

// the Corrector of fmi.h
int bwtm_corrector_create(const bwtm_kmers*, uint32_t, uint64_t, bwtm_corrector** out) { *out = nullptr; return BWTM_ENODEV; }
void bwtm_corrector_free(bwtm_corrector*) {}
uint64_t bwtm_corrector_solid(const bwtm_corrector*) { return 0; }
uint64_t bwtm_corrector_bytes(const bwtm_corrector*) { return 0; }
int bwtm_correct_batch(const bwtm_corrector*, const uint8_t*, const uint64_t*, uint64_t, uint32_t, uint8_t*, uint8_t*, uint32_t*) { return BWTM_ENODEV; }
int bwtm_correct_sequences(const bwtm_corrector*, const bwtm_index*, const uint64_t*, uint64_t, uint64_t, uint64_t, uint32_t, uint64_t*, uint8_t*, uint64_t, uint8_t*, uint32_t*)
{
  return BWTM_ENODEV;
}

}
