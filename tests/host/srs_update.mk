# The host driver of the updatable SRS (tests/test_srs_update_host.py): a plain build and one under the sanitizer flags of the Makefile
# beside it ($(SAN)), which this file includes rather than repeats.   make -f srs_update.mk srs_update_host srs_update_host_san
include Makefile
UDEPS = srs_update_host.cpp $(wildcard $(CSRC)/*.hpp)
srs_update_host: $(UDEPS)
	$(CXX) -O2 -std=c++17 -w srs_update_host.cpp -o $@
srs_update_host_san: $(UDEPS)
	$(CXX) $(SAN) srs_update_host.cpp -o $@
