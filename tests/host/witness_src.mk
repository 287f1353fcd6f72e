# The host driver of witness_src.hpp (tests/test_witness_src_host.py): a plain build and one under the sanitizer flags of the Makefile
# beside it ($(SAN)), which this file includes rather than repeats.
#   make -f witness_src.mk witness_src_host witness_src_host_san
include Makefile
WDEPS = witness_src_host.cpp $(CSRC)/witness_src.hpp $(CSRC)/field.hpp $(CSRC)/constants.hpp ../../include/sonic_hip.h
witness_src_host: $(WDEPS)
	$(CXX) -O2 -std=c++17 -w witness_src_host.cpp -o $@
witness_src_host_san: $(WDEPS)
	$(CXX) $(SAN) witness_src_host.cpp -o $@
