# The host driver of the pairing and its segmented product (tests/test_pairing_groups_host.py): a plain build and one under the sanitizer
# flags of the Makefile beside it ($(SAN)), which this file includes rather than repeats.   make -f pairing.mk pairing_host pairing_host_san
include Makefile
GDEPS = pairing_host.cpp $(wildcard $(CSRC)/*.hpp)
pairing_host: $(GDEPS)
	$(CXX) -O2 -std=c++17 -w pairing_host.cpp -o $@
pairing_host_san: $(GDEPS)
	$(CXX) $(SAN) pairing_host.cpp -o $@
