# The host driver of the subgroup tests (tests/test_subgroup_host.py): a plain build and one under the sanitizer flags of the Makefile
# beside it ($(SAN)), which this file includes rather than repeats.   make -f subgroup.mk subgroup_host subgroup_host_san
include Makefile
SDEPS = subgroup_host.cpp $(wildcard $(CSRC)/*.hpp)
subgroup_host: $(SDEPS)
	$(CXX) -O2 -std=c++17 -w subgroup_host.cpp -o $@
subgroup_host_san: $(SDEPS)
	$(CXX) $(SAN) subgroup_host.cpp -o $@
