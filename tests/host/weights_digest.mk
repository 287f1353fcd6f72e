# The host driver of weights digest v2 (tests/test_weights_digest_host.py): a plain build and one under the sanitizer flags of the Makefile
# beside it ($(SAN)), which this file includes rather than repeats.
#   make -f weights_digest.mk weights_digest_host weights_digest_host_san
include Makefile
WDEPS = weights_digest_host.cpp $(CSRC)/weights_tree.hpp $(CSRC)/witness_tree.hpp $(CSRC)/fs.hpp $(CSRC)/sha256.hpp $(CSRC)/field.hpp $(CSRC)/constants.hpp
weights_digest_host: $(WDEPS)
	$(CXX) -O2 -std=c++17 -w weights_digest_host.cpp -o $@
weights_digest_host_san: $(WDEPS)
	$(CXX) $(SAN) weights_digest_host.cpp -o $@
