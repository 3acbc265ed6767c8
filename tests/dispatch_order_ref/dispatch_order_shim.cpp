// Host shim of csrc/dispatch_order.hpp (TEST INFRASTRUCTURE ONLY): the placement functions of the SSAO and lighting launches, built
// with the host compiler by tests/test_dispatch_order.py.
#include "dispatch_order.hpp"

extern "C" {
uint32_t shim_band_of(uint32_t k, uint32_t nBands, uint32_t ways) { return cry::band_of(k, nBands, ways); }
uint32_t shim_launch_band(uint32_t k, uint32_t nBands, uint32_t ways) { return cry::launch_band(k, nBands, ways); }
uint32_t shim_light_dispatch_row(uint32_t by, uint32_t tileRows) { return cry::light_dispatch_row(by, tileRows); }
uint32_t shim_light_band_rows(void) { return cry::kLightBandRows; }
uint32_t shim_light_ways(void) { return CRY_LIGHT_BAND_WAYS; }
uint32_t shim_ssao_ways(void) { return CRY_SSAO_BAND_WAYS; }
}
