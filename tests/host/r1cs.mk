# The host driver of r1cs.hpp (tests/test_r1cs_host.py): a plain build and one under the sanitizer flags of the Makefile beside it
# ($(SAN)), which this file includes rather than repeats.
#   make -f r1cs.mk r1cs_host r1cs_host_san
include Makefile
RDEPS = r1cs_host.cpp $(CSRC)/r1cs.hpp $(CSRC)/field.hpp $(CSRC)/constants.hpp ../../include/sonic_hip.h
r1cs_host: $(RDEPS)
	$(CXX) -O2 -std=c++17 -w r1cs_host.cpp -o $@
r1cs_host_san: $(RDEPS)
	$(CXX) $(SAN) r1cs_host.cpp -o $@
